"""Static guard for the paired sweeps of the symmetric force pass (nb_force_symw_pairs, kernels/symmetric.hip.h).

A paired sweep's rotation step is two traveler-steps: per packed group of residents two crossed forms of 16 packed instructions
+ 2 v_rsq_f32 each, and 14 lane moves -- 8 v_mov_b32_dpp for the traveler dwords, 6 v_add_f32_dpp that move the 6 sum dwords on and add
what the step found to them in the same instruction -- where two single steps rotate 20.  The
gain IS that count: a swapped operand the compiler does not fold into op_sel costs a move per use, a second copy of the residents
costs 64 registers and the second wave per SIMD.  So, at build time, on the gfx950 code the library is linked from:
  * the paired loop holds exactly 32 NG packed instructions, 4 NG v_rsq_f32, 8 v_mov_b32_dpp + 6 v_add_f32_dpp and no other vector
    instruction, no memory access, no no-op;
  * the two single-sweep loops next to it keep their counts (18 NG + 10 and 14 NG + 4), in the paired kernel and in
    nb_force_symw<NG, 1>, which NB_FLAG_SINGLE_SWEEPS still launches;
  * the kernels fit 256 VGPRs (two waves per SIMD) without scratch;
  * in the built library the paired loop's head sits on a 32-byte boundary and every 64-bit instruction of it on an 8-byte one.
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

PAIRS = {4: "_ZN2nb19nb_force_symw_pairsILi4EEE", 8: "_ZN2nb19nb_force_symw_pairsILi8EEE"}
SINGLE = {4: "_ZN2nb13nb_force_symwILi4ELi1EEE", 8: "_ZN2nb13nb_force_symwILi8ELi1EEE"}


def built_asm():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    return open(ASM).read()


def rotation_loops(text, mangled):
    """The innermost loops of a kernel that rotate travelers, as lists of instruction lines (labels and comments dropped), by length."""
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
def test_paired_loop_is_the_pair_arithmetic_and_fourteen_lane_moves(ng):
    text = built_asm()
    loops = rotation_loops(text, PAIRS[ng])
    # own range and queued pieces: each of the three forms twice
    assert len(loops) == 6, [len(lp) for lp in loops]
    for lp in loops:
        assert not any(o.startswith(("scratch_", "ds_", "global_", "buffer_", "flat_")) for o in lp)
    paired = [lp for lp in loops if is_paired(lp)]
    assert len(paired) == 2
    for lp in paired:
        pk, rsq, mov, valu = counts(lp)
        add = lp.count("v_add_f32_dpp")
        assert (pk, rsq, mov, add) == (32 * ng, 4 * ng, 8, 6), (ng, pk, rsq, mov, add)
        assert sum("_dpp" in o for o in lp) == 14
        assert valu == pk + rsq + 14, (ng, sorted(set(o for o in lp if o.startswith("v_") and not o.startswith(("v_pk_", "v_rsq_f32", "v_mov_b32_dpp", "v_add_f32_dpp")))))
        assert not any(o.startswith(("v_mov_b32_e", "v_mov_b64", "v_pk_mov_b32", "v_swap")) for o in lp)
        assert "s_nop" not in lp and "s_waitcnt" not in lp
        # the loop counter behind the 64-bit instructions: decrement, compare, branch
        assert len(lp) == valu + 3 and all(o.startswith("s_") for o in lp[-3:]), lp[-4:]


@pytest.mark.parametrize("ng", [4, 8])
def test_single_sweep_loops_keep_their_counts_beside_the_paired_one(ng):
    text = built_asm()
    for mangled, nloops in ((PAIRS[ng], 6), (SINGLE[ng], 4)):
        loops = [lp for lp in rotation_loops(text, mangled) if not is_paired(lp)]
        assert len(loops) == 4 and len(rotation_loops(text, mangled)) == nloops, mangled
        for both, lp in zip((False, False, True, True), loops):
            pk, rsq, dpp, valu = counts(lp)
            per_step = 10 if both else 4
            u = dpp // per_step                       # rotation steps per trip (hipcc unrolls the short 8-resident body by 2)
            assert u >= 1 and dpp == per_step * u, (mangled, both, dpp)
            assert (pk, rsq) == ((16 if both else 12) * ng * u, 2 * ng * u) and valu == pk + rsq + dpp, (mangled, both, pk, rsq, valu)
            assert not any(o.startswith(("scratch_", "ds_", "global_", "buffer_", "flat_")) for o in lp)


def test_paired_kernels_fit_two_waves_per_simd_without_scratch():
    built_asm()
    text = open(RES).read()
    seen = 0
    for mangled in list(PAIRS.values()) + list(SINGLE.values()):
        m = re.search(r"Function Name: %s\w*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)" % mangled, text, re.S)
        assert m, mangled
        vgprs, agprs, scratch, spill = (int(x) for x in m.groups())
        assert vgprs + agprs <= 256 and scratch == 0 and spill == 0, (mangled, vgprs, agprs, scratch, spill)
        seen += 1
    assert seen == 4


def test_paired_loop_head_on_a_32_byte_boundary_in_the_built_library():
    lib = os.path.join(CSRC, "libnbody3d_hip.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("needs the built library and llvm-objdump")
    sys.path.insert(0, os.path.normpath(os.path.join(CSRC, "..", "..", "tools")))
    import loop_parity
    rows = loop_parity.loops(loop_parity.device_disassembly(lib), 64)
    for ng in (4, 8):
        # (kernel, head address, dwords, 64-bit instructions, misaligned ones, 32-bit instructions): 36 NG + 14 of 64 bits, 3 of 32
        paired = [r for r in rows if "nb_force_symw_pairsILi%dE" % ng in r[0] and r[3] == 36 * ng + 14]
        assert len(paired) == 2, (ng, [(hex(r[1]), r[2], r[3]) for r in rows if "nb_force_symw_pairsILi%dE" % ng in r[0]])
        for name, head, dwords, wide, bad, narrow in paired:
            assert head % 32 == 0 and bad == 0 and narrow == 3 and dwords == 2 * wide + 3, (ng, hex(head), dwords, wide, bad, narrow)
