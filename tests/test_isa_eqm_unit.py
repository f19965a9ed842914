"""Static guard for the equal-mass kernels with unit mass product (nb_force_symw_unit, nb_force_symw_pairs_unit; kernels/symmetric.hip.h, `UNIT`).

Where the one G*m of an equal-mass system is a power of two, the product commutes with every rounding: the loops accumulate inv * d
without it and G*m multiplies each row of sums once, where the row is stored.  A packed group and form takes 14 packed instructions
where the equal-mass kernels take 15 (tests/test_isa_eqm.py) and the general ones 16.  The gain IS that count, so, on the gfx950 code the
library is linked from:
  * the paired loop holds exactly 28 NG packed instructions, 4 NG v_rsq_f32, 6 v_mov_b32_dpp + 6 v_add_f32_dpp and no other vector
    instruction, no memory access, no no-op, no wait, and the loop counter's three instructions come last;
  * the single loops hold (14 NG, 2 NG, 9) and (11 NG, 2 NG, 3) per rotation step, in both kernels;
  * six rotation loops in the paired kernel, four in the single one;
  * the kernels fit 256 VGPRs (two waves per SIMD) without scratch;
  * in the built library the loop heads sit on 32-byte boundaries and every 64-bit instruction of the loops on an 8-byte one.
(The equal-mass kernels' own counts and names: tests/test_isa_eqm.py, unchanged; the general ones: tests/test_isa_paired_sweeps.py.)
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")
ASM = os.path.join(CSRC, "nb_engine.gfx950.s")
RES = os.path.join(CSRC, "nb_engine.resources.txt")

PAIRS = {4: "_ZN2nb24nb_force_symw_pairs_unitILi4EEE", 8: "_ZN2nb24nb_force_symw_pairs_unitILi8EEE"}
SINGLE = {4: "_ZN2nb18nb_force_symw_unitILi4ELi1EEE", 8: "_ZN2nb18nb_force_symw_unitILi8ELi1EEE"}
MEMORY = ("scratch_", "ds_", "global_", "buffer_", "flat_", "s_load", "s_buffer_load")


@pytest.fixture(scope="module")
def asm_text():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    return open(ASM).read()


def rotation_loops(text, mangled):
    """The innermost loops of a kernel that rotate travelers, as lists of opcodes (labels and comments dropped), by length."""
    m = re.search(r"^(%s\w*):.*?$(.*?)^\.Lfunc_end" % mangled, text, re.S | re.M)
    assert m, mangled
    lines = [l.split(";")[0].strip() for l in m.group(2).splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        b = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if b and b.group(1) in labels and labels[b.group(1)] < i:
            loops.append(lines[labels[b.group(1)]:i + 1])
    rot = [lp for lp in loops if any(o.startswith("v_mov_b32_dpp") for o in lp)]
    inner = [lp for lp in rot if not any(o is not lp and len(o) < len(lp) and o[0] in lp for o in rot)]
    return sorted(([l.split()[0] for l in lp if not l.endswith(":")] for lp in inner), key=len)


def counts(ops):
    valu = [o for o in ops if o.startswith("v_")]
    return sum(o.startswith("v_pk_") for o in valu), ops.count("v_rsq_f32_e64"), ops.count("v_mov_b32_dpp"), len(valu)


def is_paired(ops):
    return "v_add_f32_dpp" in ops          # only the paired loop moves its sums on with an add


@pytest.mark.parametrize("ng", [4, 8])
def test_unit_paired_loop_is_twenty_eight_packed_per_group_and_twelve_lane_moves(asm_text, ng):
    loops = rotation_loops(asm_text, PAIRS[ng])
    assert len(loops) == 6, [len(lp) for lp in loops]          # own range and queued pieces: each of the three forms twice
    paired = [lp for lp in loops if is_paired(lp)]
    assert len(paired) == 2
    for lp in paired:
        pk, rsq, mov, valu = counts(lp)
        add = lp.count("v_add_f32_dpp")
        assert (pk, rsq, mov, add) == (28 * ng, 4 * ng, 6, 6), (ng, pk, rsq, mov, add)
        assert sum("_dpp" in o for o in lp) == 12
        assert valu == pk + rsq + 12, (ng, sorted(set(o for o in lp if o.startswith("v_") and not o.startswith(("v_pk_", "v_rsq_f32", "v_mov_b32_dpp", "v_add_f32_dpp")))))
        assert not any(o.startswith(("v_mov_b32_e", "v_mov_b64", "v_pk_mov_b32", "v_swap")) for o in lp)
        assert not any(o.startswith(MEMORY) for o in lp)
        assert "s_nop" not in lp and "s_waitcnt" not in lp
        # the loop counter behind the 64-bit instructions: decrement, compare, branch
        assert len(lp) == valu + 3 and all(o.startswith("s_") for o in lp[-3:]), lp[-4:]


@pytest.mark.parametrize("ng", [4, 8])
def test_unit_single_loops_hold_no_mass_product(asm_text, ng):
    for mangled, nloops in ((PAIRS[ng], 6), (SINGLE[ng], 4)):
        every = rotation_loops(asm_text, mangled)
        loops = [lp for lp in every if not is_paired(lp)]
        assert len(loops) == 4 and len(every) == nloops, mangled
        for both, lp in zip((False, False, True, True), loops):
            pk, rsq, dpp, valu = counts(lp)
            per_step = 9 if both else 3
            u = dpp // per_step                       # rotation steps per trip (hipcc unrolls the short 8-resident body)
            assert u >= 1 and dpp == per_step * u, (mangled, both, dpp)
            assert (pk, rsq) == ((14 if both else 11) * ng * u, 2 * ng * u) and valu == pk + rsq + dpp, (mangled, both, pk, rsq, valu)
            assert not any(o.startswith(MEMORY) for o in lp) and "s_waitcnt" not in lp


def test_unit_kernels_fit_two_waves_per_simd_without_scratch(asm_text):
    text = open(RES).read()
    seen = 0
    for mangled in list(PAIRS.values()) + list(SINGLE.values()):
        m = re.search(r"Function Name: %s\w*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)" % mangled, text, re.S)
        assert m, mangled
        vgprs, agprs, scratch, spill = (int(x) for x in m.groups())
        assert vgprs + agprs <= 256 and scratch == 0 and spill == 0, (mangled, vgprs, agprs, scratch, spill)
        seen += 1
    assert seen == 4


def test_unit_loop_heads_on_32_byte_boundaries_in_the_built_library():
    lib = os.path.join(CSRC, "libnbody3d_hip.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("needs the built library and llvm-objdump")
    sys.path.insert(0, os.path.normpath(os.path.join(CSRC, "..", "..", "tools")))
    import loop_parity
    rows = loop_parity.loops(loop_parity.device_disassembly(lib), 64)
    for ng in (4, 8):
        # (kernel, head address, dwords, 64-bit instructions, misaligned ones, 32-bit instructions): the paired loop is 32 NG + 12 of 64 bits, 3 of 32
        mine = [r for r in rows if "nb_force_symw_pairs_unitILi%dE" % ng in r[0]]
        paired = [r for r in mine if r[3] == 32 * ng + 12]
        assert len(paired) == 2, (ng, [(hex(r[1]), r[2], r[3]) for r in mine])
        for name, head, dwords, wide, bad, narrow in paired:
            assert head % 32 == 0 and bad == 0 and narrow == 3 and dwords == 2 * wide + 3, (ng, hex(head), dwords, wide, bad, narrow)
        # the single forms (whole multiples of 16 NG + 9 or 13 NG + 3 instructions of 64 bits; a handful of 32-bit ones: the counter, padding),
        # twice in either kernel
        single = [r for r in rows if ("nb_force_symw_pairs_unitILi%dE" % ng in r[0] or "nb_force_symw_unitILi%dELi1E" % ng in r[0])
                  and r[5] <= 8 and (r[3] % (16 * ng + 9) == 0 or r[3] % (13 * ng + 3) == 0)]
        assert len(single) == 8, (ng, [(r[0][:40], hex(r[1]), r[3], r[5]) for r in rows if "_unitILi%dE" % ng in r[0]])
        for name, head, dwords, wide, bad, narrow in single:
            assert head % 32 == 0 and bad == 0, (name, hex(head), wide, bad)
