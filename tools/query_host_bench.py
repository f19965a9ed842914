#!/usr/bin/env python3
"""The host-side cost of the device-pointer queries the Ahmad-Cohen scheme goes through in every regular step: N = 1,024 bodies,
m = 256 points, where the host bounds the time.  Per call kind (neighbors_device, neighbor_lists_device with cap 16,
list_force_device): --calls calls, then one sync(), a host clock around the whole, after a warm-up of --warmup calls.  Prints ONE
JSON line: microseconds per call (`*_issue_us`: up to the last call's return, without the wait behind it).

--pkg DIR puts another tree's nbody3d-webgpu_amd directory in front and --lib FILE loads another library (to time the build of
another commit in turns with this one, the bindings and the library apart; profiles/r17/query_refactor.md).  Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "nbody3d-webgpu_amd"))
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--cap", type=int, default=16)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--kinds", nargs="+", default=["neighbors", "neighbor_lists", "list_force"])
    ap.add_argument("--repeat", type=int, default=1, help="timed runs per kind (the figure: the first; `*_all_us`: every one)")
    ap.add_argument("--lib", default=None, help="another libnbody3d_hip.so for the bindings to load")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if args.lib:
        os.environ["NB_ENGINE_LIB"] = os.path.abspath(args.lib)
    import torch  # first: one HIP runtime for the process
    sys.path.insert(0, os.path.abspath(args.pkg))
    from nbody3d_amd import Simulation, capi, ic

    dev = torch.device("cuda", 0)
    n, m, cap = args.n, args.m, args.cap
    b, v = ic.plummer(n, seed=7)
    pts = torch.tensor(b[:m].copy(), dtype=torch.float32, device=dev)
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    d2 = torch.empty(m, dtype=torch.float32, device=dev)
    cnt = torch.empty(m, dtype=torch.int32, device=dev)
    lst = torch.empty((m, cap), dtype=torch.int32, device=dev)
    acc = torch.empty((m, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    out = {"label": args.label, "library": capi.library_path(), "n": n, "m": m, "cap": cap, "calls": args.calls}
    with Simulation(n) as sim:
        sim.init(b, v)
        sim.set_params(1e-3, 1.0)
        p, i, d, c, l, a = (t.data_ptr() for t in (pts, idx, d2, cnt, lst, acc))
        kinds = {"neighbors": lambda: sim.neighbors_device(p, m, i, d, c, radius=0.3),
                 "neighbor_lists": lambda: sim.neighbor_lists_device(p, m, l, cap, c, radius=0.3),
                 "list_force": lambda: sim.list_force_device(l, m, cap, points_ptr=p, count_ptr=c, accel_ptr=a)}
        for name, call in kinds.items():      # (in this order: list_force reads the rows neighbor_lists wrote)
            for _ in range(args.warmup):
                call()
            sim.sync()
            if name not in args.kinds:
                continue
            runs = []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call()
                t1 = time.perf_counter()
                sim.sync()
                runs.append((round((time.perf_counter() - t0) / args.calls * 1e6, 3), round((t1 - t0) / args.calls * 1e6, 3)))
            out[name + "_us"], out[name + "_issue_us"] = runs[0]      # issue: the calls alone, without the wait behind them
            if args.repeat > 1:
                out[name + "_all_us"] = [r[0] for r in runs]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
