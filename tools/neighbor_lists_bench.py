#!/usr/bin/env python3
"""Times nb_neighbor_lists (Simulation.neighbor_lists_device: NB_NBR_DEVICE, so no host copy is in the number) with device events
around warmed calls on the handle's own stream, and prints ONE JSON line.

  per precision (f32, f64) and per M = N in --sizes (default 65,536 and 262,144), a Plummer sphere, the bodies' own positions
  (AT_BODIES), in ONE process on ONE handle, in turns:
      lists            list + count, cap = 128, the radius chosen (bisection on nb_neighbors' own count) for a mean count of ~32
      nearest_count    nb_neighbors index + dist2 + count with the same radius -- the yardstick: existing code, the count pass itself
      lists_dense      unbarred: mean count ~128, cap = 256 (the slow path dominates)
  `ratio_lists` = lists / nearest_count (of the best times; the medians are in the line too).  `truncated` = the share of rows with
  count > cap; `slow_groups` = the share of (wave, 4-row group) pairs of the f32 fill pass in which some lane has a member, i.e.
  that take the slow path -- counted on the host from the rows the call returned (members past cap are not in them: a slight
  under-count where rows are truncated).

The bar is computed, not guessed: `loops` holds the VALU instructions of the built plain (unmasked) inner loop of the count pass
(nb_nbr_pk<true>) and of the fill pass's fast path (nb_nbl_pk: the group loop up to the branch around the stores) from
csrc/nb_engine.gfx950.s (`make asm`), their issue cycles by DESIGN.md section 7.1's convention (packed and plain VALU 4 cycles),
PER PAIR since the two loops are unrolled over different numbers of rows, and bar = (count + fill) / count x 1.20.  `--loops-only` prints just that and needs no GPU.

Every figure: at least --min-seconds of the same work before the timed run and in it; --rounds timed runs per figure, interleaved
across the arms; the JSON holds the best, the median and the spread (max - min) / min.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import re
import sys

import numpy as np

try:
    import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
except Exception as e:    # pragma: no cover
    sys.exit("neighbor_lists_bench: torch is required for the device buffers and events: %s" % e)

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


def _loops(text, kernel):
    """The loops of `kernel` in the built code, each as its lines from the label a backward branch goes to up to that branch."""
    m = re.search(r"^(_ZN2nb\d+%s\w*):.*?$(.*?)^\.Lfunc_end" % re.escape(kernel), text, re.S | re.M)
    lines = [l.split(";")[0].strip() for l in m.group(2).splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        b = re.match(r"s_c?branch\w*\s+(\S+)", l)
        if b and b.group(1) in labels and labels[b.group(1)] < i:
            loops.append(lines[labels[b.group(1)]:i + 1])
    return loops


def _tally(lp):
    valu = [re.sub(r"_e(32|64)$", "", l.split()[0]) for l in lp if l.startswith("v_")]
    mix = {}
    for o in valu:
        mix[o] = mix.get(o, 0) + 1
    pairs = mix.get("v_pk_fma_f32", 0)            # two v_pk_fma_f32 per two pairs: one per pair
    salu = len([l for l in lp if l.startswith("s_") and not l.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch"))])
    return {"mix": mix, "valu": len(valu), "salu": salu, "branches": len([l for l in lp if l.startswith(("s_cbranch", "s_branch"))]),
            "lds_reads": len([l for l in lp if l.startswith("ds_read")]), "stores": len([l for l in lp if l.startswith("global_store")]),
            "pairs": pairs, "cycles": 4 * len(valu), "cycles_per_pair": 4.0 * len(valu) / max(1, pairs)}


def plain_loop(text, kernel):
    """Tally of the longest innermost loop of `kernel` that computes distances (v_pk_fma_f32), is unmasked (no v_cmp_eq / v_cmp_ne on
    indices) and holds no store.  For the fill pass that is its fast path: the back edge is the branch around the slow path."""
    loops = _loops(text, kernel)
    inner = [lp for lp in loops if not any(o is not lp and len(o) < len(lp) and o[0] in lp for o in loops)]
    plain = [lp for lp in inner if any(o.startswith("v_pk_fma_f32") for o in lp) and not any(re.match(r"v_cmp_(ne|eq)_u32", o) for o in lp)
             and not any(o.startswith("global_store") for o in lp)]
    return max(plain, key=len)


def loop_counts():
    path = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc", "nb_engine.gfx950.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    fast = plain_loop(text, "nb_nbl_pk")
    # the same loop with its slow path: the longest loop around the fast path that reads no more tile rows than it does
    reads = len([o for o in fast if o.startswith("ds_read")])
    whole = max([lp for lp in _loops(text, "nb_nbl_pk") if fast[0] in lp and any(o.startswith("global_store") for o in lp)
                 and len([o for o in lp if o.startswith("ds_read")]) == reads], key=len)
    at = whole.index(fast[0])
    slow = whole[:at] + whole[at + len(fast):]
    out = {"count_pass": _tally(plain_loop(text, "nb_nbr_pkILb1E")), "fill_fast_path": _tally(fast), "fill_slow_path": _tally(slow)}
    out["cycle_ratio_lists"] = (out["count_pass"]["cycles_per_pair"] + out["fill_fast_path"]["cycles_per_pair"]) / out["count_pass"]["cycles_per_pair"]
    out["bar_lists"] = 1.20 * out["cycle_ratio_lists"]
    return out


def slow_group_share(lists, n, j_rows=4):
    """Share of the f32 fill pass's (wave, group of 4 rows) pairs with a member: a wave holds the points p0 + 256 q + lane, q = 0..3,
    lane in [64 w, 64 w + 64) of the block at p0 = 1,024 x block; the groups of a chunk start at multiples of 4 (whole tiles)."""
    m, cap = lists.shape
    k, c = np.nonzero(lists != 0xffffffff)
    j = lists[k, c].astype(np.int64)
    wave = (k // 1024) * 4 + (k % 256) // 64
    hit = np.unique(wave * ((n + j_rows - 1) // j_rows) + j // j_rows)
    waves = ((m + 1023) // 1024) * 4
    return len(hit) / float(waves * ((n + j_rows - 1) // j_rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops-only", action="store_true", help="print the loop counts and the bar from csrc/nb_engine.gfx950.s; no GPU")
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32", "f64"])
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense (mean count ~128, cap 256) case")
    args = ap.parse_args()
    if args.loops_only:
        print(json.dumps({"tool": "neighbor_lists_bench", "loops": loop_counts()}))
        return
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("neighbor_lists_bench: no GPU")
    stream = torch.cuda.Stream()
    out = {"tool": "neighbor_lists_bench", "device": torch.cuda.get_device_name(0), "min_seconds": args.min_seconds, "rounds": args.rounds,
           "loops": loop_counts(), "cases": []}

    def timed(fn):
        """ms per call of fn (enqueues on `stream`): estimate, warm for min_seconds, then one timed run of min_seconds."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(); stream.synchronize()
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        reps = max(2, int(np.ceil(args.min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
        for _ in range(reps):
            fn()
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1) / reps

    for precision in args.precisions:
        dt, tt = (np.float64, torch.float64) if precision == "f64" else (np.float32, torch.float32)
        for n in args.sizes:
            b, v = ic.plummer(n, seed=7)
            with Simulation(n, precision=precision, stream=stream.cuda_stream) as s:
                s.init(b.astype(dt), v.astype(dt))
                s.set_params(1e-3, 1.0)
                with torch.cuda.stream(stream):
                    idx = torch.zeros(n, device="cuda", dtype=torch.int32)
                    cnt = torch.zeros(n, device="cuda", dtype=torch.int32)
                    d2 = torch.zeros(n, device="cuda", dtype=tt)
                    lst = torch.zeros((n, 256), device="cuda", dtype=torch.int32)

                def mean_count(h):
                    s.neighbors_device(None, 0, None, None, cnt.data_ptr(), bodies=(0, n), radius=h)
                    stream.synchronize()
                    return float(cnt.double().mean().item())

                def radius_for(target):          # bisection: the mean count grows with the radius
                    lo, hi = 0.0, 4.0
                    for _ in range(24):
                        mid = 0.5 * (lo + hi)
                        lo, hi = (mid, hi) if mean_count(mid) < target else (lo, mid)
                    return 0.5 * (lo + hi)

                case = {"precision": precision, "n": n, "shape": s.neighbor_lists_shape(n, 128)}
                setups = [("lists", 32.0, 128)] + ([] if args.no_dense else [("lists_dense", 128.0, 256)])
                arms = {}
                for name, target, cap in setups:
                    h = radius_for(target)
                    s.neighbor_lists_device(None, 0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=h)
                    stream.synchronize()
                    c = cnt.cpu().numpy().astype(np.int64)
                    case[name] = {"radius": h, "cap": cap, "mean_count": float(c.mean()), "max_count": int(c.max()),
                                  "truncated": float((c > cap).mean())}
                    if precision == "f32":
                        rows = lst.view(-1)[:n * cap].view(n, cap).cpu().numpy().view(np.uint32)
                        case[name]["slow_groups"] = slow_group_share(rows, n)
                    arms[name] = (lambda h=h, cap=cap: s.neighbor_lists_device(None, 0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=h))
                    arms["nearest_count" + name[5:]] = (lambda h=h: s.neighbors_device(None, 0, idx.data_ptr(), d2.data_ptr(), cnt.data_ptr(), bodies=(0, n), radius=h))
                ms = {k: [] for k in arms}
                for _ in range(args.rounds):
                    for k, fn in arms.items():
                        ms[k].append(timed(fn))
                for k, xs in ms.items():
                    case[k + "_ms"] = {"best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}
                for name, _, _ in setups:
                    ref = "nearest_count" + name[5:]
                    case["ratio_" + name] = min(ms[name]) / min(ms[ref])
                    case["ratio_" + name + "_median"] = float(np.median(ms[name]) / np.median(ms[ref]))
                out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
