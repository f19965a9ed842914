#!/usr/bin/env python3
"""Times nb_split_force (Simulation.split_force_device: NB_SPLIT_DEVICE, so no host copy is in the number) against the force+jerk pass of
the SAME Hermite handle, and prints ONE JSON line.

  The bar comes from the built loops (`make asm` -> csrc/nb_engine.gfx950.s): the VALU and transcendental instructions of one trip of
  the plain inner loop of nb_split_pk<.., true> and of nb_fj_pk, their issue cycles by DESIGN.md section 7.1's convention (every VALU
  instruction 4 cycles, a transcendental 8), PER PAIR since the two kernels hold different numbers of points per lane, and
  bar = (split cycles per pair / force+jerk cycles per pair) x 1.20.  `--loops-only` prints just that and needs no GPU.

  per precision (f32, f64) and per M = N in --sizes (default 65,536 and 262,144): ic.plummer(N, seed=7) on a Hermite handle, AT_BODIES,
  device pointers, the radius chosen (bisection on nb_neighbors' count) for a mean count of ~32.  In ONE process on ONE handle, in
  turns, --rounds times:
      split        nb_split_force, all four outputs                             -- the main figure
      full_pass    nb_force_pass(1): the existing force+jerk pass over all N x N pairs -- the baseline
      split_accel  the accel pair alone (no velocity tile, no jerk arithmetic)
      lists        nb_neighbor_lists, cap 128  \\  with full_pass the route this call replaces: `route` = full_pass + lists +
      list_force   nb_list_force, a + jerk     /   list_force
  Reported per arm: ms best / median / spread; `ratio` = split / full_pass of the best times and of the medians, `ratio_worse` the
  larger of the two, `inside_bar` (f32 only: the bar is the f32 loops'); `ratio_accel`, `ratio_route` = split / route.
  `clock`: what the runtime and a read-only rocm-smi --showclocks report when the tool starts.

Every figure: at least --min-seconds of the same work before the timed run and in it.  Every GPU step runs under its own time limit
(--step-limit seconds): when one runs out the process ends with status 124 and starts nothing more.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import threading

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ASM = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc", "nb_engine.gfx950.s")
TRANS = ("v_rsq_f32", "v_rsq_f64", "v_rcp_f32", "v_sqrt_f32")


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


def plain_loop(text, kernel):
    """Tally of the innermost loop of `kernel` that holds the pair arithmetic (the one with the most reciprocal roots)."""
    loops = _loops(text, kernel)
    inner = [lp for lp in loops if not any(o is not lp and len(o) < len(lp) and o[0] in lp for o in loops)]
    lp = max(inner, key=lambda q: len([o for o in q if o.startswith("v_rsq")]))
    valu = [re.sub(r"_e(32|64)$", "", l.split()[0]) for l in lp if l.startswith("v_")]
    mix = {}
    for o in valu:
        mix[o] = mix.get(o, 0) + 1
    trans = sum(mix.get(t, 0) for t in TRANS)
    pairs = mix.get("v_rsq_f32", 0)               # one reciprocal root per pair
    cycles = 4 * len(valu) + 4 * trans
    return {"mix": mix, "valu": len(valu), "transcendental": trans, "pairs": pairs, "lds_reads": len([l for l in lp if l.startswith("ds_read")]),
            "cycles": cycles, "cycles_per_pair": cycles / float(max(1, pairs))}


def loop_counts():
    if not os.path.exists(ASM):
        return None
    text = open(ASM).read()
    ng = int(re.search(r"^_ZN2nb\d+nb_split_pkILi(\d)ELb1E", text, re.M).group(1))      # the points per lane the library was built with: 2 x ng
    out = {"split_ng": ng, "split_jerk": plain_loop(text, "nb_split_pkILi%dELb1E" % ng), "split_accel": plain_loop(text, "nb_split_pkILi%dELb0E" % ng),
           "force_jerk": plain_loop(text, "nb_fj_pkILi2E")}
    out["cycle_ratio"] = out["split_jerk"]["cycles_per_pair"] / out["force_jerk"]["cycles_per_pair"]
    out["bar"] = 1.20 * out["cycle_ratio"]
    return out


class step_limit:
    """A time limit for one GPU step: a step that outlives it ends the process (status 124); nothing more is started."""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self._expire, (what, seconds))
        self.t.daemon = True

    @staticmethod
    def _expire(what, seconds):
        sys.stderr.write("split_force_bench: step '%s' exceeded its limit of %g s; ending\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *a):
        self.t.cancel()


def device_clock(torch):
    """What can be read of the device and its clocks without changing anything (tools/list_force_bench.py has the same report)."""
    p = torch.cuda.get_device_properties(0)
    out = {"arch": getattr(p, "gcnArchName", None), "compute_units": p.multi_processor_count}
    khz = getattr(p, "clock_rate", None)
    if khz:
        out["max_engine_clock_mhz"] = khz / 1e3
    smi = shutil.which("rocm-smi") or ("/opt/rocm/bin/rocm-smi" if os.path.exists("/opt/rocm/bin/rocm-smi") else None)
    if smi:
        try:
            r = subprocess.run([smi, "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=20)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            out["rocm_smi_showclocks"] = json.loads(line[-1]) if line else None
        except Exception as e:      # a report only: the figures do not depend on it
            out["rocm_smi_showclocks"] = "unavailable: %s" % type(e).__name__
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops-only", action="store_true", help="print the loop counts and the bar from csrc/nb_engine.gfx950.s; no GPU")
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32", "f64"])
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=60.0)
    args = ap.parse_args()
    if args.loops_only:
        print(json.dumps({"tool": "split_force_bench", "loops": loop_counts()}))
        return
    try:
        import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
    except Exception as e:    # pragma: no cover
        sys.exit("split_force_bench: torch is required for the device buffers and events: %s" % e)
    sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
    from nbody3d_amd import Simulation, capi, ic
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("split_force_bench: no GPU")
    stream = torch.cuda.Stream()
    loops = loop_counts()
    out = {"tool": "split_force_bench", "device": torch.cuda.get_device_name(0), "clock": device_clock(torch), "min_seconds": args.min_seconds,
           "rounds": args.rounds, "loops": loops, "cases": []}

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
            with Simulation(n, precision=precision, stream=stream.cuda_stream, integrator="hermite4") as s:
                s.init(b.astype(dt), v.astype(dt))
                s.set_params(1e-3, 1.0)
                with torch.cuda.stream(stream):
                    cnt = torch.zeros(n, device="cuda", dtype=torch.int32)
                    o = [torch.zeros((n, 4), device="cuda", dtype=tt) for _ in range(4)]
                    lst = torch.zeros((n, 128), device="cuda", dtype=torch.int32)

                def mean_count(h):
                    s.neighbors_device(None, 0, None, None, cnt.data_ptr(), bodies=(0, n), radius=h)
                    stream.synchronize()
                    return float(cnt.double().mean().item())

                with step_limit(args.step_limit, "radius"):
                    lo, hi = 0.0, 4.0
                    for _ in range(24):          # bisection: the mean count grows with the radius
                        mid = 0.5 * (lo + hi)
                        lo, hi = (mid, hi) if mean_count(mid) < 32.0 else (lo, mid)
                    h = 0.5 * (lo + hi)
                    mc = mean_count(h)
                case = {"precision": precision, "n": n, "radius": h, "mean_count": mc, "shape": s.split_force_shape(n)}
                arms = {
                    "split": lambda: s.split_force_device(0, bodies=(0, n), radius=h, accel_irr_ptr=o[0].data_ptr(), accel_reg_ptr=o[1].data_ptr(),
                                                          jerk_irr_ptr=o[2].data_ptr(), jerk_reg_ptr=o[3].data_ptr()),
                    "full_pass": None,              # nb_force_pass times itself
                    "split_accel": lambda: s.split_force_device(0, bodies=(0, n), radius=h, accel_irr_ptr=o[0].data_ptr(), accel_reg_ptr=o[1].data_ptr()),
                    "lists": lambda: s.neighbor_lists_device(None, 0, lst.data_ptr(), 128, cnt.data_ptr(), bodies=(0, n), radius=h),
                    "list_force": lambda: s.list_force_device(lst.data_ptr(), 0, 128, bodies=(0, n), count_ptr=cnt.data_ptr(), accel_ptr=o[0].data_ptr(),
                                                              jerk_ptr=o[2].data_ptr()),
                }
                with step_limit(args.step_limit, "warm-up"):
                    full_reps = max(2, int(np.ceil(args.min_seconds * 1e3 / max(s.force_pass(1), 1e-3))))
                    arms["lists"](); stream.synchronize()
                ms = {k: [] for k in arms}
                for _ in range(args.rounds):
                    for k, fn in arms.items():
                        with step_limit(args.step_limit, "%s %s n=%d" % (k, precision, n)):
                            if fn is None:
                                s.force_pass(full_reps)
                                ms[k].append(s.force_pass(full_reps))
                            else:
                                ms[k].append(timed(fn))
                for k, xs in ms.items():
                    case[k + "_ms"] = {"best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}
                med = lambda k: float(np.median(ms[k]))
                case["ratio"] = min(ms["split"]) / min(ms["full_pass"])
                case["ratio_median"] = med("split") / med("full_pass")
                case["ratio_worse"] = max(case["ratio"], case["ratio_median"])
                case["ratio_accel"] = min(ms["split_accel"]) / min(ms["full_pass"])
                case["route_ms"] = min(ms["full_pass"]) + min(ms["lists"]) + min(ms["list_force"])
                case["ratio_route"] = min(ms["split"]) / case["route_ms"]
                if precision == "f32" and loops:
                    case["bar"] = loops["bar"]
                    case["inside_bar"] = bool(case["ratio_worse"] <= loops["bar"])
                out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
