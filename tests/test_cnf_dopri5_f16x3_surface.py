"""The surface of the f16x3 adaptive point-CNF solve, without a GPU: header, binding, configuration switch, build list, audit."""
import os

import pytest

ROOT = os.path.join(os.path.dirname(__file__), "..")
NEW = "ode_dp5_f16x3w.hip"


def test_header_declares_and_lib_binds_the_entries():
    from caspr_amd import lib
    hdr = open(os.path.join(ROOT, "include", "caspr_hip.h")).read()
    for name in ("caspr_cnf_dopri5_h3_ws_bytes", "caspr_cnf_dopri5_h3_f32"):
        assert name + "(" in hdr and name in lib.SIGNATURES
    # caspr_cnf_dopri5_f32 without e / logp_in / logp_out, plus the status word; the parent entry keeps its 31 arguments
    assert len(lib.SIGNATURES["caspr_cnf_dopri5_h3_f32"][1]) == 31 - 3 + 1
    assert len(lib.SIGNATURES["caspr_cnf_dopri5_f32"][1]) == 31
    assert len(lib.SIGNATURES["caspr_cnf_dopri5_h3_ws_bytes"][1]) == 3
    decl = hdr[hdr.index("int caspr_cnf_dopri5_h3_f32("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == 29 and "unsigned *status" in decl and "logp" not in decl


def test_the_switch_defaults_to_bf16x6_and_is_validated_where_it_is_read(monkeypatch):
    from caspr_amd import config, ops
    assert config.KernelConfig().cnf_dp5_split == "bf16x6" and config.KernelConfig().cnf_split == "f16x3"
    assert ops.CNF_DP5_SPLIT == "bf16x6" and ops.cnf_dp5_split() == "bf16x6"
    assert config.active()["cnf_dp5_split"] == "bf16x6"
    monkeypatch.setattr(ops, "CNF_DP5_SPLIT", "f16x3")
    assert ops.cnf_dp5_split() == "f16x3" and config.active()["cnf_dp5_split"] == "f16x3"
    monkeypatch.setattr(ops, "CNF_DP5_SPLIT", "f16x4")
    with pytest.raises(ValueError, match="CNF_DP5_SPLIT"):
        ops.cnf_dp5_split()


def test_the_environment_knob_needs_debug():
    import warnings
    from caspr_amd import config
    assert config.load({"CASPR_DEBUG": "1", "CASPR_CNF_DP5_SPLIT": "F16x3 "}).cnf_dp5_split == "f16x3"
    with pytest.raises(ValueError, match="CASPR_CNF_DP5_SPLIT"):
        config.load({"CASPR_DEBUG": "1", "CASPR_CNF_DP5_SPLIT": "fp8"})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert config.load({"CASPR_CNF_DP5_SPLIT": "f16x3"}).cnf_dp5_split == "bf16x6"
    assert any("CASPR_CNF_DP5_SPLIT" in str(w.message) for w in caught)


def test_build_list_and_audit_carry_the_new_file():
    from caspr_amd.csrc import audit, build
    assert NEW in build.SOURCES and build.EXTRA[NEW] == build.EXTRA["ode_f16x3w.hip"]
    assert audit.AUDITS[NEW] is audit.audit_cnf_dp5_h3w
    assert os.path.exists(os.path.join(ROOT, "caspr_amd", "csrc", NEW))


def test_the_stage_body_is_one_text_and_every_fragment_is_a_build_dependency():
    import glob
    from caspr_amd.csrc import build
    csrc = os.path.join(ROOT, "caspr_amd", "csrc")
    frag = "ode_h3w_eval.inc"
    for f in ("ode_f16x3w.hip", NEW):
        assert '#include "%s"' % frag in open(os.path.join(csrc, f)).read()
    # the f16x3 CNF sources: the two kernels' files and what is shared between them
    srcs = ["ode_f16x3w.hip", NEW] + sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "ode_h3w*")))
    assert frag in srcs
    for stmt in ("auto region_a = ", "auto l2_step = ", "auto piece_head = "):
        assert [f for f in srcs if stmt in open(os.path.join(csrc, f)).read()] == [frag], stmt
    deps = {os.path.abspath(p) for p in build.deps()}
    shared = {os.path.abspath(p) for p in glob.glob(os.path.join(csrc, "*")) if p.endswith((".h", ".inc"))}
    assert os.path.abspath(os.path.join(csrc, frag)) in shared and shared <= deps


def test_each_controller_text_exists_once_and_every_shared_file_is_a_build_dependency():
    """What the three adaptive solves share (dp5_tables.inc, dp5_rules.h, dp5.h; common.h: the moving batch norm): each marker of the
    tableau, the step-size rule, the interpolant and the batch-norm transform occurs in exactly one file of csrc, the shared one."""
    import glob
    from caspr_amd.csrc import build
    csrc = os.path.join(ROOT, "caspr_amd", "csrc")
    text = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(csrc, "*")) if p.endswith((".hip", ".h", ".inc"))}
    where = lambda lit: sorted(f for f, t in text.items() if lit in t)
    assert where("19372.0 / 6561") == ["dp5_tables.inc"]
    assert where("6025192743.0") == ["dp5_tables.inc"]
    assert where("powf(sqrtf(r), 0.2f)") == ["dp5_rules.h"]
    assert where("18.0 * y0d") == ["dp5_rules.h"] and text["dp5_rules.h"].count("18.0 * y0d") == 1
    assert where("expf(-0.5f * logf(") == ["common.h"]
    for f in ("ode_dp5.hip", NEW, "ode_latent_dp5.hip"):
        assert '#include "dp5_tables.inc"' in text[f], f
        assert '#include "dp5_rules.h"' in text[f] or '#include "dp5.h"' in text[f], f
    assert '#include "dp5_rules.h"' in text["dp5.h"]
    deps = {os.path.abspath(p) for p in build.deps()}
    for f in ("dp5_tables.inc", "dp5_rules.h", "dp5.h"):
        assert os.path.abspath(os.path.join(csrc, f)) in deps, f


def test_state_dict_key_surface_is_unchanged(monkeypatch):
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    keys = sorted(CaSPR().state_dict())
    monkeypatch.setattr(ops, "CNF_DP5_SPLIT", "f16x3")
    m = CaSPR(cnf_method="dopri5")
    assert sorted(m.state_dict()) == keys
    assert m.point_cnf.chain[1].last_dp5_kernel is None


def test_code_object_audit_of_the_in_tree_object():
    from caspr_amd.csrc import audit
    obj = os.path.join(ROOT, "caspr_amd", "csrc", NEW.replace(".hip", ".o"))
    if not (os.path.exists(obj) and audit.tools_present()):
        pytest.skip("no in-tree object (run build()) or no LLVM tools")
    res = audit.audit_cnf_dp5_h3w(obj)
    assert res["accvgpr_reads"] == 512 and res["accvgpr_writes"] == 512 and res["mfma_on_acc"] == 192
    rk4 = os.path.join(ROOT, "caspr_amd", "csrc", "ode_f16x3w.o")
    if os.path.exists(rk4):       # ONE copy of the stage body: the counts of the RK4 kernel
        ref = audit.audit_cnf_h3w(rk4)
        assert (res["mfma"], res["cvt_pk"]) == (ref["mfma"], ref["cvt_pk"])
