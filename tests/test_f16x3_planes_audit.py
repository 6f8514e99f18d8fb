"""Code-object audit of what the f16x3 point-CNF kernel (csrc/ode_f16x3w.hip) does in passes 1-3 of layer 2, on the CPU: the accumulator
file holds the two f16 planes of hidden layer 1's activations, so those passes read plane words and split nothing."""
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


def test_passes_1_to_3_split_nothing(kernel):
    """The kernel's 960 MFMAs in program order: 192 of layer 1's loop body, 384 of pass 0, 384 of the passes-1-3 body.  Between the
    577th and the 960th there is no conversion to f16, no compare and no select: a plane word goes from its accumulator read to the
    MFMA untouched (248 reads there; the 8 of k-step 0 sit in front of the 577th)."""
    mf = [i for i, s in enumerate(kernel) if s.startswith("v_mfma")]
    assert len(mf) == 960
    body = kernel[mf[576]:mf[959] + 1]
    hits = [s for s in body if re.match(r"v_cvt_pk_f16_f32|v_cndmask|v_cmp", s)]
    assert not hits, "%d split instructions in the passes-1-3 body, e.g. %s" % (len(hits), hits[:3])
    assert sum(1 for s in body if s.startswith("v_accvgpr_read_b32")) == 248
    assert not any(s.startswith("v_accvgpr_write_b32") for s in body)


def test_split_count():
    """304 v_cvt_pk_f16_f32 in the kernel, two (one per plane) for every value pair the source splits: 8 pairs of layer 1's chunk 0 up
    front + 16 in its loop body (eight pieces x two pairs) + 128 in pass 0 of layer 2 (all 256 activations of a lane, once) = 152 pairs,
    and none in passes 1-3.  The kernel that split the activations again in passes 1-3 had 128 pairs more there (560).  The second
    variant of the change (the residual by a mixed-precision FMA reading the f16 half) was measured and not kept; it removes conversions
    FROM f16, not these, so the figure is the same either way."""
    from caspr_amd.csrc import audit
    if not (os.path.exists(OBJ) and audit.tools_present()):
        pytest.skip("needs the in-tree object and the ROCm LLVM tools")
    r = audit.audit_cnf_h3w(OBJ)
    assert r["cvt_pk"] == 304, r
    assert r["accvgpr_reads"] == 512 and r["accvgpr_writes"] == 512, r
