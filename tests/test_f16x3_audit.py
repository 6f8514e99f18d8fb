"""Code-object audit of the f16x3 point-CNF kernel (csrc/ode_f16x3w.hip), on the CPU: the same contract as
test_host_cpu.test_cnf_x6w_kernel_keeps_its_accumulator_file_to_itself for the kernel it was copied from."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cnf_h3w_kernel_keeps_its_accumulator_file_to_itself():
    """cnf_rk4_h3w_kernel manages a0..a255 by hand through inline asm; hipcc must keep out of them and must not spill (a scratch reload
    would also drain the LDS-DMA queue with vmcnt(0)).  The check lives in caspr_amd/csrc/audit.py and ALSO runs inside build() before
    the library is linked; here it runs on the in-tree object."""
    from caspr_amd.csrc import audit
    obj = os.path.join(ROOT, "caspr_amd", "csrc", "ode_f16x3w.o")
    if not (os.path.exists(obj) and audit.tools_present()):
        pytest.skip("needs the in-tree object and the ROCm LLVM tools")
    r = audit.audit_cnf_h3w(obj)
    assert r["accvgpr_reads"] == 512 and r["accvgpr_writes"] == 512 and r["mfma_on_acc"] == 192 and r["mfma"] == 960, r


def test_the_build_audits_the_new_object():
    from caspr_amd.csrc import audit, build
    assert "ode_f16x3w.hip" in build.SOURCES and audit.AUDITS["ode_f16x3w.hip"] is audit.audit_cnf_h3w
    assert "-amdgpu-mfma-vgpr-form" in build.EXTRA["ode_f16x3w.hip"] and "-packed-fp32-ops" in build.FLAGS
