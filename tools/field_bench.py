#!/usr/bin/env python3
"""Times nb_field_eval (Simulation.field_device: NB_FIELD_DEVICE, so no host copy is in the number) with device events around
warmed calls on the handle's own stream, and prints ONE JSON line.

  big shape     f32, M = N = 262,144, the bodies' own positions (AT_BODIES): both outputs / acceleration only / potential only,
                in turns with the ordered-pair force pass of the same system on the same device (nb_force_pass on a
                NB_FLAG_NO_SYM handle: the same pair loop without the potential) -- `ratio_*` = field time / force-pass time
  small M       pairs/s at (m = 1,024, N = 1,048,576) and (m = 4,096, N = 262,144) beside the big shape's
  fp64          f64 handle and NB_FIELD_F64 on the f32 handle at m = 4,096, N = 262,144
  host form     wall time of field(bodies=(0, N)) with host arrays at M = N = 262,144 and the share of it that is not the kernels

Every figure: at least --min-seconds (default 0.5) of the same work before the timed run and in it; --rounds (default 3) timed
runs per figure, interleaved across the figures of a group; the JSON holds the best and the median.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

try:
    import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
except Exception as e:    # pragma: no cover
    sys.exit("field_bench: torch is required for the device buffers and events: %s" % e)

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--n-large", type=int, default=1048576)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--only-big", action="store_true", help="the big shape against the force pass, nothing else")
    args = ap.parse_args()
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("field_bench: no GPU")
    stream = torch.cuda.Stream()
    out = {"tool": "field_bench", "device": torch.cuda.get_device_name(0), "n": args.n, "min_seconds": args.min_seconds, "rounds": args.rounds}

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

    def group(arms):
        """arms: {name: callable returning ms}; `rounds` interleaved runs -> {name: {best_ms, median_ms, all_ms}}"""
        got = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                got[k].append(fn())
        return {k: {"best_ms": min(v), "median_ms": float(np.median(v)), "all_ms": v} for k, v in got.items()}

    def dev(shape, dtype):
        with torch.cuda.stream(stream):
            return torch.zeros(shape, device="cuda", dtype=dtype)

    n = args.n
    b, v = ic.plummer(n, seed=1)
    with Simulation(n, flags=capi.NB_FLAG_NO_SYM, stream=stream.cuda_stream) as s:
        s.init(b, v)
        s.set_params(1e-3, 1.0)
        out["baseline_variant"] = s.variant
        acc, phi = dev((n, 4), torch.float32), dev((n,), torch.float32)

        def force_pass():
            est = s.force_pass(2)
            reps = max(2, int(np.ceil(args.min_seconds * 1e3 / est)))
            s.force_pass(reps)
            return s.force_pass(reps)

        big = group({
            "force_pass": force_pass,
            "field_both": lambda: timed(lambda: s.field_device(None, 0, acc.data_ptr(), phi.data_ptr(), bodies=(0, n))),
            "field_accel": lambda: timed(lambda: s.field_device(None, 0, acc.data_ptr(), None, bodies=(0, n))),
            "field_phi": lambda: timed(lambda: s.field_device(None, 0, None, phi.data_ptr(), bodies=(0, n))),
        })
        out["big"] = big
        for k in ("both", "accel", "phi"):
            out["ratio_" + k] = big["field_" + k]["median_ms"] / big["force_pass"]["median_ms"]
            out["ratio_%s_best" % k] = big["field_" + k]["best_ms"] / big["force_pass"]["best_ms"]
        pairs_big = float(n) * n / (big["field_both"]["median_ms"] * 1e-3)
        out["pairs_per_s_big"] = pairs_big

        if args.only_big:
            print(json.dumps(out))
            return

        # small M against the same system, and the fp64 mode
        m = 4096
        rng = np.random.default_rng(11)
        lo, hi = b[:, :3].min(0), b[:, :3].max(0)
        pts = np.zeros((m, 4), np.float32)
        pts[:, :3] = lo + (hi - lo) * rng.random((m, 3))
        with torch.cuda.stream(stream):
            tp = torch.from_numpy(pts).to("cuda")
        a4, p4 = dev((m, 4), torch.float32), dev((m,), torch.float32)
        a8, p8 = dev((m, 4), torch.float64), dev((m,), torch.float64)
        small = group({
            "m4096_f32": lambda: timed(lambda: s.field_device(tp.data_ptr(), m, a4.data_ptr(), p4.data_ptr())),
            "m4096_fp64_mode": lambda: timed(lambda: s.field_device(tp.data_ptr(), m, a8.data_ptr(), p8.data_ptr(), f64=True)),
        })
        out["small"] = small
        out["pairs_per_s_m4096"] = float(m) * n / (small["m4096_f32"]["median_ms"] * 1e-3)
        out["pairs_per_s_m4096_fp64_mode"] = float(m) * n / (small["m4096_fp64_mode"]["median_ms"] * 1e-3)

        # host-pointer form: wall time of the whole call against the device time of the same request
        s.field(bodies=(0, n))
        walls = []
        for _ in range(max(3, args.rounds)):
            t0 = time.perf_counter()
            s.field(bodies=(0, n))
            walls.append((time.perf_counter() - t0) * 1e3)
        out["host_form_wall_ms"] = float(np.median(walls))
        out["host_form_copy_share"] = max(0.0, 1.0 - big["field_both"]["median_ms"] / out["host_form_wall_ms"])

    with Simulation(n, precision="f64", stream=stream.cuda_stream) as s:
        s.init(b.astype(np.float64), v.astype(np.float64))
        s.set_params(1e-3, 1.0)
        with torch.cuda.stream(stream):
            tp8 = torch.from_numpy(pts.astype(np.float64)).to("cuda")
        r = group({"m4096_f64_handle": lambda: timed(lambda: s.field_device(tp8.data_ptr(), m, a8.data_ptr(), p8.data_ptr()))})
        out["small"].update(r)
        out["pairs_per_s_m4096_f64_handle"] = float(m) * n / (r["m4096_f64_handle"]["median_ms"] * 1e-3)

    if not args.skip_large:
        nl, ml = args.n_large, 1024
        bl, vl = ic.plummer(nl, seed=3)
        with Simulation(nl, flags=capi.NB_FLAG_NO_SYM, stream=stream.cuda_stream) as s:
            s.init(bl, vl)
            s.set_params(1e-3, 1.0)
            r = group({"m1024_n_large": lambda: timed(lambda: s.field_device(tp.data_ptr(), ml, a4.data_ptr(), p4.data_ptr()))})
            out["small"].update(r)
            out["n_large"] = nl
            out["pairs_per_s_m1024_n_large"] = float(ml) * nl / (r["m1024_n_large"]["median_ms"] * 1e-3)
            out["small_m_ratio_m1024"] = out["pairs_per_s_m1024_n_large"] / pairs_big
    out["small_m_ratio_m4096"] = out["pairs_per_s_m4096"] / pairs_big
    print(json.dumps(out))


if __name__ == "__main__":
    main()
