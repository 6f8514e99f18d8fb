"""Code-object audit of the instruction stream of the f16x3 point-CNF kernel (csrc/ode_f16x3w.hip) after "the wave's instruction
stream" (DESIGN.md 3), on the CPU, on the in-tree object: issue slots the result does not need stay out."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "caspr_amd", "csrc", "ode_f16x3w.o")


@pytest.fixture(scope="module")
def kernel():
    from caspr_amd.csrc import audit
    if not (os.path.exists(OBJ) and audit.tools_present()):
        pytest.skip("needs the in-tree object and the ROCm LLVM tools")
    notes, dis = audit._code_object(OBJ)
    return audit._kernel(notes, dis, "_Z18cnf_rk4_h3w_kernel9CnfH3Args")[1]


def test_no_compare_and_select_under_the_first_576_mfmas(kernel):
    """Layer 1's loop body and pass 0 of layer 2 (the 1st to the 576th MFMA in program order) split 144 value pairs; the flush of their
    f16-subnormal plane values is done on the plane word with packed 16-bit integer operations (three per first-plane word, three and a
    v_and_b32 per second-plane word), not by a v_cmp / v_cndmask pair per value through the one VCC."""
    mf = [i for i, s in enumerate(kernel) if s.startswith("v_mfma")]
    assert len(mf) == 960
    body = kernel[mf[0]:mf[575] + 1]
    hits = [s for s in body if re.match(r"v_cmp|v_cndmask", s)]
    assert not hits, "%d compares / selects between the first and the 576th MFMA, e.g. %s" % (len(hits), hits[:3])
    for op in ("v_pk_lshrrev_b16", "v_pk_min_u16", "v_pk_mul_lo_u16"):
        assert sum(1 for s in body if s.startswith(op)) == 2 * 144, op


def test_pads_and_scalar_instructions(kernel):
    """Pinned with the tested compiler (audit.TESTED_HIPCC) at what this build has; the parent's figures beside them:
      * s_nop in the whole kernel: 656 (parent 932).  276 fewer: no pad between a compare and its select, none inside an LDS-DMA statement
        (the M0 write sits one MFMA ahead of the load);
      * scalar instructions other than s_nop / s_waitcnt between the 577th and the 960th MFMA, the body of passes 1-3: 149 (parent
        293).  One source address and one M0 write per 16 KB piece instead of four of each."""
    mf = [i for i, s in enumerate(kernel) if s.startswith("v_mfma")]
    assert len(mf) == 960
    assert sum(1 for s in kernel if s.startswith("s_nop")) == 656
    body = kernel[mf[576]:mf[959] + 1]
    assert sum(1 for s in body if re.match(r"s_(?!nop|waitcnt)", s)) == 149
    assert not any(s.startswith("s_nop") for s in body)


def test_m0_once_per_piece():
    """47 M0 writes for 188 LDS-DMA instructions: one per piece (7 pieces in the prologue, 8 in layer 1's loop body, 16 in each of the two
    layer-2 bodies), the four loads of a wave's share told apart by the immediate offset; audit_cnf_h3w checks that nothing else
    touches M0 and that no load sits directly behind its M0 write."""
    from caspr_amd.csrc import audit
    if not (os.path.exists(OBJ) and audit.tools_present()):
        pytest.skip("needs the in-tree object and the ROCm LLVM tools")
    r = audit.audit_cnf_h3w(OBJ)
    assert r["lds_dma"] == 188 and r["m0_writes"] == 47, r
