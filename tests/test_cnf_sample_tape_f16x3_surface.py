"""The surface of the f16x3 sampling solve with the tape (csrc/ode_sample_tape_h3w.hip, config.cnf_tape_split), without a GPU: header,
binding, exported symbols, build list, audit registration, the configuration switch, the deferred channel's message, the audit of the
in-tree object."""
import ctypes
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(__file__), "..")
NEW = "ode_sample_tape_h3w.hip"
ENTRIES = ("caspr_cnf_sample_tape_h3_f32", "caspr_cnf_sample_tape_h3_frames_f32")


def test_header_declares_lib_binds_and_the_library_exports_the_entries():
    from caspr_amd import lib
    hdr = open(os.path.join(ROOT, "include", "caspr_hip_train.h")).read()
    for name, parent in zip(ENTRIES, ("caspr_cnf_sample_tape_f32", "caspr_cnf_sample_tape_frames_f32")):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared in include/caspr_hip_train.h" % name
        assert "unsigned *status" in m.group(1) and "w1h" in m.group(1) and "w2h" in m.group(1)
        # the parent entry's arguments plus the status word
        assert len(lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == len(lib.SIGNATURES[parent][1]) + 1
    so = os.path.join(ROOT, "caspr_amd", "csrc", "libcaspr_hip.so")
    if os.path.exists(so):
        L = ctypes.CDLL(so)
        for name in ENTRIES:
            assert hasattr(L, name), "%s is not exported by the built library" % name
    pub = open(os.path.join(ROOT, "include", "caspr_hip.h")).read()
    assert re.search(r"\b4 caspr_cnf_sample_tape_h3_f32", pub), "the status word's value 4 is not documented beside 1 and 2"


def test_build_list_and_audit_carry_the_new_file():
    from caspr_amd.csrc import audit, build
    assert NEW in build.SOURCES and build.EXTRA[NEW] == build.EXTRA["ode_f16x3w.hip"]
    assert audit.AUDITS[NEW] is audit.audit_cnf_sample_tape_h3w
    src = open(os.path.join(ROOT, "caspr_amd", "csrc", NEW)).read()
    for frag in ("ode_h3w.h", "ode_h3w_setup.inc", "ode_h3w_ring.inc", "ode_h3w_eval.inc"):
        assert '#include "%s"' % frag in src, frag


def test_wrappers_and_routing_exist():
    from caspr_amd import train_ops as T
    from caspr_amd.train import flow_grad as FG
    assert callable(T.cnf_sample_tape_h3) and callable(T.cnf_sample_tape_h3_frames)
    x6, h3 = object(), object()
    pair = FG._SolvePacks(x6, h3)
    assert FG._sample_tape_route(x6, x6, 1024) == (False, x6, x6)          # no f16x3 packs handed in: today's launch at any n
    assert FG._sample_tape_route(pair, pair, 127) == (False, x6, x6)       # the 64-point fallback


def test_the_switch_defaults_to_bf16x6_and_is_validated_where_it_is_read(monkeypatch):
    from caspr_amd import config, ops
    from caspr_amd.train import flow_grad as FG
    assert config.KernelConfig().cnf_tape_split == "bf16x6"
    assert ops.CNF_TAPE_SPLIT == "bf16x6" and ops.cnf_tape_split() == "bf16x6"
    assert config.active()["cnf_tape_split"] == "bf16x6"
    x6, h3 = object(), object()
    pair = FG._SolvePacks(x6, h3)
    assert FG._sample_tape_route(pair, pair, 128) == (False, x6, x6)
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x3")
    assert ops.cnf_tape_split() == "f16x3" and config.active()["cnf_tape_split"] == "f16x3"
    assert FG._sample_tape_route(pair, pair, 128) == (True, h3, h3)
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x4")
    with pytest.raises(ValueError, match="CNF_TAPE_SPLIT"):
        ops.cnf_tape_split()


def test_the_environment_knob_needs_debug():
    import warnings
    from caspr_amd import config
    assert config.load({"CASPR_DEBUG": "1", "CASPR_CNF_TAPE_SPLIT": "F16x3 "}).cnf_tape_split == "f16x3"
    with pytest.raises(ValueError, match="CASPR_CNF_TAPE_SPLIT"):
        config.load({"CASPR_DEBUG": "1", "CASPR_CNF_TAPE_SPLIT": "fp8"})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert config.load({"CASPR_CNF_TAPE_SPLIT": "f16x3"}).cnf_tape_split == "bf16x6"
    assert any("CASPR_CNF_TAPE_SPLIT" in str(w.message) for w in caught)


def test_the_channel_names_the_entry_and_its_remedy():
    from caspr_amd import lib, ops
    with pytest.raises(lib.CasprHipError) as e:
        ops._cnf_h3_report([([4], None)])
    assert "caspr_cnf_sample_tape_h3_f32" in str(e.value) and 'cnf_tape_split="bf16x6"' in str(e.value)
    assert "cnf_dp5_split" not in str(e.value) and 'cnf_split="bf16x6"' not in str(e.value)
    for word in (1, 2, 3):
        with pytest.raises(lib.CasprHipError) as e:
            ops._cnf_h3_report([([word], None)])
        assert "cnf_tape_split" not in str(e.value), word
    with pytest.raises(lib.CasprHipError) as e:
        ops._cnf_h3_report([([1], None), ([4], None)])
    assert 'cnf_split="bf16x6"' in str(e.value) and 'cnf_tape_split="bf16x6"' in str(e.value)
    ops._cnf_h3_report([([0], None)])


def test_code_object_audit_of_the_in_tree_object():
    from caspr_amd.csrc import audit
    obj = os.path.join(ROOT, "caspr_amd", "csrc", NEW.replace(".hip", ".o"))
    if not (os.path.exists(obj) and audit.tools_present()):
        pytest.skip("no in-tree object (run build()) or no LLVM tools")
    res = audit.audit_cnf_sample_tape_h3w(obj)
    assert res["accvgpr_reads"] == 512 and res["accvgpr_writes"] == 512 and res["mfma_on_acc"] == 192
    assert res["vgpr_count"] is not None and res["vgpr_count"] <= 512
    rk4 = os.path.join(ROOT, "caspr_amd", "csrc", "ode_f16x3w.o")
    if os.path.exists(rk4):       # the same evaluation text in the same instruction stream: the counts of the inference kernel
        ref = audit.audit_cnf_h3w(rk4)
        for key in ("accvgpr_reads", "accvgpr_writes", "mfma", "mfma_on_acc", "lds_dma", "m0_writes", "cvt_pk"):
            assert res[key] == ref[key], (key, res[key], ref[key])
