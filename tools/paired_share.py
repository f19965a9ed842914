#!/usr/bin/env python3
"""Which share of a plan's chunk-sweeps does nb_force_symw_pairs run two at a time?  (CPU only: the planner's answer, walked as the
kernel walks it -- kernels/symmetric.hip.h, `pair`.)  A paired sweep issues 151 instead of 154 vector instructions per rotation step
with 16 residents per lane (8 residents: 79 instead of 82), an own-chunk sweep 116 (60): the predicted ratio of SQ_INSTS_VALU.
The equal-mass kernels issue 142 (74), 145 (77) and 115 (59): the second ratio, against the paired kernel.
The equal-mass kernels with unit mass product (form 2: G*m a power of two) issue 134 (70), 137 (73) and 107 (55): the third ratio, against
the equal-mass kernels (form 1) -- what SQ_INSTS_VALU of the force kernel should show between the two forms.
    python tools/paired_share.py [N ...] [--variant V]"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import capi  # noqa: E402

args = sys.argv[1:]
variant = int(args[args.index("--variant") + 1]) if "--variant" in args else 0
sizes = [int(a) for a in args if a.isdigit() and args[max(0, args.index(a) - 1)] != "--variant"] or [65536, 131072, 262144, 1048576]
for n in sizes:
    q = capi.plan_query(n, force_variant=variant)
    pl, ups, ng = q["plan"], q["ups"], q["ipl"] // 2
    if not q["symw"] or q["x"] != 3 or ng not in (4, 8):
        print("N=%d %s: no paired kernel for this shape" % (n, q["variant"]))
        continue
    cps, nsb, th, tl, n_hi, zc = 2 * ng, pl["nsb"], pl["total_hi"], pl["total_lo"], pl["n_hi"], pl["zc"]
    first_lo = n_hi * th
    first_z = first_lo + (nsb - n_hi) * tl
    ranges = [(int(a), int(b)) for a, b, _, _ in q["waves"]] + [(int(u), int(u) + (int(l) >> 16)) for u, l in q["pieces"]]
    paired = single = own = 0.0
    for u, uend in ranges:
        while u < uend:
            p = u // ups
            if p < first_lo:
                g = p // th; k = p - g * th; total = th
            elif p < first_z:
                r = p - first_lo; g = n_hi + r // tl; k = r - (g - n_hi) * tl; total = tl
            else:
                g = nsb; k = p - first_z; total = zc
            both_end = total - cps if g < nsb else 0
            ug_end = min((p - k + total) * ups, uend)
            while u < ug_end:
                q0 = u % ups
                if q0 == 0 and ug_end - u >= 2 * ups and k + 1 < both_end:
                    paired += 2; u += 2 * ups; k += 2
                    continue
                nun = min(ups - q0, ug_end - u)
                if k < both_end:
                    single += nun / ups
                else:
                    own += nun / ups
                u += nun
                if u % ups == 0:
                    k += 1
    tot = paired + single + own
    both, lone = 18 * ng + 10, 14 * ng + 4
    before = (paired + single) * both + own * lone
    after = paired * (both - 3) + single * both + own * lone
    # the equal-mass kernels (nb_force_symw_pairs_eqm): one mass product and one lane move less per traveler-step, against `after`
    eqm = paired * (both - 3 - ng - 1) + single * (both - ng - 1) + own * (lone - 1)
    # ... with unit mass product (nb_force_symw_pairs_unit): no mass product at all, one packed instruction less per group and form, against `eqm`
    unit = paired * (both - 3 - 2 * ng - 1) + single * (both - 2 * ng - 1) + own * (lone - ng - 1)
    print("N=%8d %-40s sweeps %9.0f: paired %.4f  single with sums %.4f  own chunks %.4f | predicted VALU instructions x %.5f | equal masses x %.5f"
          " | unit mass product (form 2 / form 1) x %.5f" % (
              n, q["variant"], tot, paired / tot, single / tot, own / tot, after / before, eqm / after, unit / eqm))
