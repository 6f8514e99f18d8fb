"""The code object of the f16x3 conv (csrc/gemm_f16x3w.hip): the hand-managed accumulator file is touched by nobody but the source, and
a chunk is 96 f16 MFMAs -- half the bf16x6 kernel's 192."""
import os

import pytest

from caspr_amd.csrc import audit

OBJ = os.path.join(os.path.dirname(audit.__file__), "gemm_f16x3w.o")


def test_conv_h3w_kernel_keeps_its_accumulator_file_to_itself():
    if not (os.path.exists(OBJ) and audit.tools_present()):
        pytest.skip("needs the in-tree object and the ROCm LLVM tools")
    res = audit.audit_conv_h3w(OBJ)
    assert len(res) == 4                                   # FUSED x STATS
    for r in res:
        assert r["accvgpr_writes"] == 768 and r["accvgpr_reads"] == 512 and r["mfma"] == 2 * 96, r
        # one v_cvt_pk_f16_f32 per value pair and plane: 8 pairs x 2 planes in the prologue and in each of the two chunk bodies
        assert r["cvt_pk"] == 3 * 16, r
    assert audit.AUDITS["gemm_f16x3w.hip"] is audit.audit_conv_h3w
