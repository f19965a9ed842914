#!/usr/bin/env python3
"""Times nb_list_force (Simulation.list_force_device: NB_LISTF_DEVICE, so no host copy is in the number) with device events around
warmed calls on the handle's own stream, and prints ONE JSON line.

  per precision (f32, f64) and per M = N in --sizes (default 65,536 and 262,144): a Plummer sphere on a Hermite handle, the rows of
  nb_neighbor_lists on the device for the bodies' own positions (AT_BODIES), cap = 128, the radius chosen (bisection on nb_neighbors'
  count) for a mean count of ~32.  In ONE process on ONE handle, in turns, --rounds times:
      a_jerk           nb_list_force, accel + jerk, count given          -- the main figure
      full_pass        nb_force_pass(1): the force+jerk pass over all N x N pairs -- the only way to the same kind of sum without this
                       call, existing code
      lists            the nb_neighbor_lists call that made the rows
      a_jerk_nocount   the same without count (every row is read to cap: the padding costs its index loads and gathers of row 0)
      a_only           accel alone, count given
      dense            unless --no-dense: mean count ~128, cap = 256, accel + jerk, count given
      knn6             short rows: accel + jerk over nb_knn's rows of the 6 nearest bodies (cap = 6, no count)
  Reported per arm: ms best / median / spread (max - min) / min; for the list arms entries/s (the valid entries: sum of min(count,
  cap)) and bytes/s at 4 + 32 bytes per entry (index + position row + velocity row; 4 + 16 for a_only); `ratio_full` = a_jerk /
  full_pass and `ratio_lists` = a_jerk / lists, of the best times, the medians beside them.
  `pass` = a_jerk is faster than full_pass at every size: the one condition (a condition in kind: a list pass slower than the pass over
  all pairs would have no point).  Everything else is recorded, not gated.

The lanes-per-row A/B: run the tool once per library and turn, the libraries alternating, NB_ENGINE_LIB=<a build with
-DNB_LF_LANES=8|16|32>; `lanes_per_row` (per case: the constant is one per precision) and `library` in the line say which build
answered.  `clock`: what the runtime and a read-only rocm-smi --showclocks report when the tool starts.

Every figure: at least --min-seconds of the same work before the timed run and in it.  Every GPU step (a setup, one timed arm) runs
under its own time limit (--step-limit seconds): when one runs out the process ends with status 124 and starts nothing more.  Needs
a GPU (no fallback)."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import threading

import numpy as np

try:
    import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
except Exception as e:    # pragma: no cover
    sys.exit("list_force_bench: torch is required for the device buffers and events: %s" % e)

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


class step_limit:
    """A time limit for one GPU step: a step that outlives it ends the process (status 124); nothing more is started."""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self._expire, (what, seconds))
        self.t.daemon = True

    @staticmethod
    def _expire(what, seconds):
        sys.stderr.write("list_force_bench: step '%s' exceeded its limit of %g s; ending\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *a):
        self.t.cancel()


def library_name():
    """Which library answers: "tree" (the built tree's) or NB_ENGINE_LIB relative to the repository (never an absolute path: the
    record is kept)."""
    lib = os.environ.get("NB_ENGINE_LIB")
    if not lib:
        return "tree"
    rel = os.path.relpath(os.path.abspath(lib), ROOT)
    return os.path.basename(lib) if rel.startswith("..") else rel


def device_clock():
    """What can be read of the device and its clocks without changing anything: the properties the runtime reports (architecture, CUs,
    the maximum engine clock in MHz where the binding has it) and, where rocm-smi is installed, its read-only --showclocks report at
    the moment the tool starts (the idle levels: the clock under load is not sampled)."""
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32", "f64"])
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=60.0)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense (mean count ~128, cap 256) case")
    ap.add_argument("--main-only", action="store_true", help="only a_jerk, full_pass, lists and knn6 (the lanes-per-row A/B)")
    args = ap.parse_args()
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("list_force_bench: no GPU")
    stream = torch.cuda.Stream()
    out = {"tool": "list_force_bench", "device": torch.cuda.get_device_name(0), "clock": device_clock(), "library": library_name(),
           "min_seconds": args.min_seconds, "rounds": args.rounds, "cases": []}

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
                    acc = torch.zeros((n, 4), device="cuda", dtype=tt)
                    jrk = torch.zeros((n, 4), device="cuda", dtype=tt)
                    lst = {128: torch.zeros((n, 128), device="cuda", dtype=torch.int32)}
                    knn6 = torch.zeros((n, 6), device="cuda", dtype=torch.int32)
                    cnts = {128: torch.zeros(n, device="cuda", dtype=torch.int32)}
                    if not (args.no_dense or args.main_only):
                        lst[256] = torch.zeros((n, 256), device="cuda", dtype=torch.int32)
                        cnts[256] = torch.zeros(n, device="cuda", dtype=torch.int32)

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

                case = {"precision": precision, "n": n, "shape": s.list_force_shape(n, 128)}
                out["lanes_per_row"] = case["shape"]["lanes_per_row"]
                setups = [("main", 32.0, 128)] + ([] if args.no_dense or args.main_only else [("dense", 128.0, 256)])
                arms, entries, bytes_per = {}, {}, {}
                for name, target, cap in setups:
                    with step_limit(args.step_limit, "rows " + name):
                        h = radius_for(target)
                        s.neighbor_lists_device(None, 0, lst[cap].data_ptr(), cap, cnts[cap].data_ptr(), bodies=(0, n), radius=h)
                        stream.synchronize()
                        c = cnts[cap].cpu().numpy().astype(np.int64)
                    valid = int(np.minimum(c, cap).sum())
                    case["rows_" + name] = {"radius": h, "cap": cap, "mean_count": float(c.mean()), "max_count": int(c.max()),
                                            "truncated": float((c > cap).mean()), "entries": valid}

                    def lf(cap=cap, count=True, jerk=True):
                        s.list_force_device(lst[cap].data_ptr(), 0, cap, bodies=(0, n), count_ptr=cnts[cap].data_ptr() if count else None,
                                            accel_ptr=acc.data_ptr(), jerk_ptr=jrk.data_ptr() if jerk else None)

                    if name == "main":
                        arms["a_jerk"] = lf
                        arms["full_pass"] = None              # nb_force_pass times itself
                        arms["lists"] = (lambda h=h, cap=cap: s.neighbor_lists_device(None, 0, lst[cap].data_ptr(), cap, cnts[cap].data_ptr(),
                                                                                       bodies=(0, n), radius=h))
                        entries["a_jerk"], bytes_per["a_jerk"] = valid, 36
                        if not args.main_only:
                            arms["a_jerk_nocount"] = (lambda lf=lf: lf(count=False))      # (lf bound now: the dense setup defines another)
                            arms["a_only"] = (lambda lf=lf: lf(jerk=False))
                            entries["a_jerk_nocount"], bytes_per["a_jerk_nocount"] = valid, 36
                            entries["a_only"], bytes_per["a_only"] = valid, 20
                    else:
                        arms["dense"] = lf
                        entries["dense"], bytes_per["dense"] = valid, 36
                with step_limit(args.step_limit, "rows knn6"):      # short rows: the 6 nearest bodies of every body, no count
                    s.knn_device(None, 0, 6, knn6.data_ptr(), None, bodies=(0, n))
                    stream.synchronize()
                arms["knn6"] = (lambda: s.list_force_device(knn6.data_ptr(), 0, 6, bodies=(0, n), accel_ptr=acc.data_ptr(), jerk_ptr=jrk.data_ptr()))
                entries["knn6"], bytes_per["knn6"] = 6 * n, 36
                with step_limit(args.step_limit, "full pass warm-up"):
                    full_reps = max(2, int(np.ceil(args.min_seconds * 1e3 / max(s.force_pass(1), 1e-3))))
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
                    if k in entries:
                        case[k + "_entries_per_s"] = entries[k] / (min(xs) * 1e-3)
                        case[k + "_bytes_per_s"] = entries[k] * bytes_per[k] / (min(xs) * 1e-3)
                case["ratio_full"] = min(ms["a_jerk"]) / min(ms["full_pass"])
                case["ratio_full_median"] = float(np.median(ms["a_jerk"]) / np.median(ms["full_pass"]))
                case["ratio_lists"] = min(ms["a_jerk"]) / min(ms["lists"])
                case["ratio_lists_median"] = float(np.median(ms["a_jerk"]) / np.median(ms["lists"]))
                case["faster_than_full_pass"] = bool(max(ms["a_jerk"]) < min(ms["full_pass"]))
                out["cases"].append(case)
    out["pass"] = all(c["faster_than_full_pass"] for c in out["cases"])
    print(json.dumps(out))
    sys.exit(0 if out["pass"] else 1)


if __name__ == "__main__":
    main()
