"""What the tests of the encounter watch inside batched block steps (nb_set_block_batch_watch) share: the engine's chunk rule of the
small pass restated, which block steps of a frozen level set a slot runs, the level sets of the census, the brute force over a
few rows of a large lattice, ties between quarters and tiles found from the brute force, and the reader of the built kernels.
Imported by test_encounter_batch_cpu.py, test_encounter_batch_gpu.py and test_encounter_batch_node.py; not a test module."""
import os
import re
import shutil
import subprocess

import numpy as np

import encounter_ref as E

TILE = 256


def bb_shape(n, cus):
    """nb_engine.hip's bb_shape: (j-chunks, bodies per chunk) of the small pass -- one chunk of whole tiles per CU."""
    tiles = E.ceil_div(n, TILE)
    c = max(1, min(cus, tiles))
    per = E.ceil_div(tiles, c) * TILE
    return E.ceil_div(n, per), per


def active_counts(lev, L=E.LATTICE_L):
    """|A| at the ticks 1 .. 2^L of one outer step with frozen levels."""
    lev = np.asarray(lev, np.int64)
    return [int((t % (1 << (L - lev)) == 0).sum()) for t in range(1, (1 << L) + 1)]


def expected_path(lev, small_max, L=E.LATTICE_L):
    """(small steps, host steps) of one outer step: a block step is small when 0 < |A| <= small_max and it is not the last one."""
    counts = active_counts(lev, L)
    small = sum(1 for t, c in enumerate(counts, 1) if 0 < c <= small_max and t != (1 << L))
    return small, len(counts) - small


# the bodies the small-set level sets of the census put at level 3: the origin where padding rows sit (0) with its neighbour (1),
# both ends of every coincident pair of E.lattice(1025), and two bodies whose smallest rho^2 is tied between quarters of one tile
CORE = (0, 1, 5, 10, 60, 64, 67, 300, 301, 700, 1023, 1024)


def small_set_levels(n, deep, mid):
    """`deep` bodies at level 3 (CORE first, then bodies spread over the system), `mid` at level 2, ONE at level 1, the rest at
    level 0: |A| = deep at the odd ticks, deep + mid at ticks 2 and 6, deep + mid + 1 at tick 4, n at tick 8."""
    assert n == 1025
    lev = np.zeros(n, np.uint8)
    core = list(CORE[:deep])
    rest = [i for i in np.linspace(2, n - 3, 4 * (deep + mid + 1)).astype(np.int64) if i not in CORE]
    rest = list(dict.fromkeys(rest))
    d = core + rest[:deep - len(core)]
    m = rest[deep - len(core):deep - len(core) + mid]
    one = rest[deep - len(core) + mid]
    lev[d], lev[m], lev[one] = 3, 2, 1
    assert (lev == 3).sum() == deep and (lev == 2).sum() == mid and (lev == 1).sum() == 1
    return lev


def rows_brute(b, rows, radius2):
    """lattice_brute for a few rows of a large lattice: for every listed row the candidate (j != i by index, integer d2 < radius2)
    of smallest d2, equal d2 to the smallest index.  Returns (rho2, partner); +inf / NONE where there is none."""
    x = np.asarray(b)[:, :3].astype(np.int64)
    rho2, partner = np.full(len(rows), np.inf), np.full(len(rows), E.NONE, np.uint32)
    big = np.iinfo(np.int64).max
    for k, i in enumerate(rows):
        d = x - x[i]
        d2 = (d * d).sum(1)
        d2[i] = big
        d2[d2 >= radius2] = big
        j = int(d2.argmin())
        if d2[j] != big:
            rho2[k], partner[k] = d2[j] + E.LATTICE_EPS2, j
    return rho2, partner


def ties(b, radii):
    """Bodies whose smallest admissible d2 is reached by several j: (between different 64-row quarters of ONE 256-row tile,
    between different tiles).  From integer distances."""
    x = np.asarray(b)[:, :3].astype(np.int64)
    n = len(x)
    thr = np.ceil(np.asarray(radii, np.float64) ** 2).astype(np.int64)
    quarter, tile = [], []
    for i in range(n):
        d = x - x[i]
        d2 = (d * d).sum(1)
        d2[i] = np.iinfo(np.int64).max
        m = d2.min()
        if m >= thr[i]:
            continue
        js = np.nonzero(d2 == m)[0]
        if len(js) > 1:
            if len(set(js // TILE)) > 1:
                tile.append(i)
            elif len(set(js // 64)) > 1:
                quarter.append(i)
    return quarter, tile


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
_built = {}


def built(csrc):
    """(assembly text, {kernel: body}, {kernel: resources}) of `make asm`, every nb:: kernel."""
    if not _built:
        import pytest
        if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
            pytest.skip("hipcc not available")
        subprocess.check_call(["make", "-C", csrc, "-s", "asm"])
        text = open(os.path.join(csrc, "nb_engine.gfx950.s")).read()
        res = open(os.path.join(csrc, "nb_engine.resources.txt")).read()
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
        rep = {}
        for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S):
            if "Function Name" not in m.group(2):
                field = lambda k: int(re.search(re.escape(k) + r": (\d+)", m.group(2)).group(1))
                rep[m.group(1)] = dict(scratch=field("ScratchSize [bytes/lane]"), vgprs=field(" VGPRs"), agprs=field("AGPRs"),
                                       occupancy=field("Occupancy [waves/SIMD]"), lds=int(m.group(3)))
        _built["k"] = (text, bodies, rep)
    return _built["k"]


def no_hit_path(body, root):
    """The instructions of one trip round the innermost loop on the path WITHOUT a hit: from a skip of the slow path
    (s_cbranch_vccz, taken), following unconditional branches and back edges, until the walk returns to where it began; the loop
    is the one that holds `root` (v_rsq_f32 | v_rsq_f64)."""
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    for start in (i for i, l in enumerate(lines) if l.startswith("s_cbranch_vccz")):
        i, ops = start, []
        for _ in range(5000):
            l = lines[i]
            if not l.endswith(":"):
                ops.append(l.split()[0])
            m = re.match(r"(s_cbranch_vccz|s_branch|s_cbranch_scc[01])\s+(\S+)", l)
            if m and m.group(2) in labels and (not m.group(1).startswith("s_cbranch_scc") or labels[m.group(2)] < i):
                i = labels[m.group(2)]      # a skip of the slow path, a jump, a back edge: taken; the loop's exit: not
            else:
                i += 1
            if i == start:
                if any(o.startswith(root) for o in ops):
                    return ops
                break
            if i >= len(lines):
                break
    raise AssertionError("no loop found behind a skip of the slow path")
