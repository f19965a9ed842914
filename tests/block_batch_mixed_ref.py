"""What test_block_batch_mixed_cpu.py and test_block_batch_mixed_gpu.py share: the two-tile census system of the small double-single
pass (nb_set_block_batch_mixed; kernels/block_batch_mixed.hip.h), the chunk rule it is built on, and the census condition.  Not a
test module."""
import numpy as np

import mixed_ref as M

CUS = 256                         # compute units of an MI355X: what the CPU test builds the system for
TILE = 256
ACTIVE = 64                       # bodies 0 .. 63 at level 1, the rest at level 0
HEAVY = 64.0                      # a census row carries this many times the common mass
DT = 2.0 ** -4                    # the outer step; the small step at tick 1 is over h = DT / 2
EPS2 = 1e-4


def bb_shape(n, cus):
    """The j-chunks of a small pass, as the engine's bb_shape: one chunk of whole tiles per CU.  (chunks, rows per chunk)"""
    tiles = -(-n // TILE)
    c = max(1, min(cus, tiles))
    per = -(-tiles // c) * TILE
    return -(-n // per), per


def two_tile_system(cus=CUS):
    """n = 256 x CUs + 257: 512 rows per chunk, so every chunk sweeps two tiles through the double-buffered loop and the last chunk is
    ragged (257 rows).  A census as well: HEAVY x the common mass at offsets 0, 63, 64, 255, 256 and 511 of chunk 0 (both ends of a
    wave's quarter, of a tile and of the chunk), at the last row of the last full chunk and at every row of the ragged one.  The
    positions keep their float64 bits (non-zero lo words from the shift).  (n, bodies, vel, levels, heavy rows)"""
    from nbody3d_amd import ic
    n = TILE * cus + TILE + 1
    chunks, per = bb_shape(n, cus)
    assert per == 2 * TILE and n - (chunks - 1) * per == TILE + 1, (n, chunks, per)
    b0, v0 = [np.array(z, np.float64) for z in ic.plummer(n, seed=21)]
    b0[:, :3] += np.asarray(M.SHIFT) * 2.0 ** -3 + 1e-9
    heavy = np.array([0, 63, 64, 255, 256, 511, (chunks - 1) * per - 1] + list(range((chunks - 1) * per, n)), np.int64)
    b0[heavy, 3] *= HEAVY
    lev = np.zeros(n, np.uint8)
    lev[:ACTIVE] = 1
    return n, b0, v0, lev, heavy


def census_moves(system):
    """Per heavy row k: how far leaving that ONE row out of the small pass (or adding it twice: the same size, the other sign) moves
    the corrected velocity of the most affected active body, as norm_err measures it (max |delta| over max |v| of the active rows).
    The row's pair terms on the active rows are fj_mixed's with fp64 sums, at the uploaded state (the predicted one is h v = 2 % of the
    system's size away); the corrector takes (a1, j1) into v by h / 2 a1 - h^2 / 12 j1."""
    n, b0, v0, lev, heavy = system
    act = np.nonzero(lev == 1)[0]
    h = DT / 2
    scale = np.abs(v0[act, :3]).max()
    moves = np.zeros(len(heavy))
    for q, k in enumerate(heavy):
        rows = np.append(act, k)
        b, v = b0[rows].copy(), v0[rows].copy()
        b[:len(act), 3] = 0.0      # the active rows add +-0: what is left is row k's term on each of them
        a, j = M.fj_mixed(b, v, 1.0, EPS2, rows=np.arange(len(act)), acc="fp64")
        moves[q] = np.abs(h / 2 * a - h * h / 12 * j).max() / scale
    return moves
