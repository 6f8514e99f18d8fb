"""The point-CNF front-end (caspr_amd/ops.py: cnf_rk4, cnf_dopri5; caspr_amd/train_ops.py: the training forward and the four tape
wrappers; train/flow_grad.py: _sample_tape_route) as a dispatch, on the CPU: which entry each call reaches, with which arguments in
which order, where the f16x3 status scope and the timer sit around the launch, and every error's type and text, against the transcript
the front-end gave before it was rewritten around one route table (tests/golden/cnf_dispatch_parent.json; cnf_dispatch_cases.py says
how it was made)."""
import os

import pytest

import cnf_dispatch_cases as D
from caspr_amd import lib

GOLDEN = D.load(os.path.join(os.path.dirname(__file__), "golden", "cnf_dispatch_parent.json"))
FLAT = [line for lines in GOLDEN.values() for line in lines]
ENTRIES = {n for n in lib.SIGNATURES if n.startswith(("caspr_cnf_rk4", "caspr_cnf_dopri5", "caspr_cnf_sample_tape", "caspr_cnf_train_fwd"))}
LAUNCHES = {n for n in ENTRIES if not n.endswith("_bytes")}
HEAD = 1 + 13            # a launch line: the entry's name, then y, hyper, ldh, tcol, w0, b0, w1, b1, w2, b2, w3, b3, H


def test_the_golden_file_is_the_case_table():
    assert list(GOLDEN) == [c.name for c in D.CASES]
    assert 80 <= len(D.CASES) <= 400


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_transcript(name):
    got = D.transcript(D.BY_NAME[name])
    assert "unknown" not in str(got), "a pointer that belongs to no tensor of the call"
    assert got == GOLDEN[name]


def test_every_entry_of_the_front_end_is_reached():
    """The twelve solve entries of lib.SIGNATURES (and the two workspace sizes that share their prefix)."""
    assert len(LAUNCHES) == 12
    seen = {line[0] for line in FLAT}
    assert ENTRIES <= seen, sorted(ENTRIES - seen)


def test_every_error_of_the_front_end_is_reached():
    texts = [line[2] for line in FLAT if line[0] == "raise"]
    starts = ["cnf_rk4: a step table is for the sampling direction only", "cnf_rk4: a step table needs the bf16x6 weight packs",
              "cnf_rk4: max_steps must lie in 1..4096, got 4097", "cnf_rk4: out (2, 129, 3) on cpu does not match y",
              "cnf_rk4: order / max_steps / out come with a step table", "cnf_rk4: w1h / w2h must be the packs of pack_cnf_h3",
              "cnf_rk4: steps must be an int32 tensor on the GPU, got int", "cnf_rk4: steps lives on meta, the samples on cpu",
              "cnf_rk4: steps must be a contiguous int32 (BT,) tensor with BT = 2, got torch.int64",
              "cnf_rk4: order must be a contiguous int32 (BT,) tensor with BT = 2, got torch.int32 (1,)",
              "cnf_dopri5: the bf16x6 weight packs w1x / w2x (pack_cnf_x6) are required", "cnf_dopri5: rtol and atol must be positive and finite",
              "cnf_dopri5: t_end must be positive and finite", "cnf_dopri5: max_attempts must be positive", "cnf_dopri5: no gradient through",
              "cnf_dopri5: the host loop reads the device", "cnf_dopri5: w1h / w2h must be the packs of pack_cnf_h3",
              "expected float32, got torch.float64", "expected a contiguous tensor"]
    for fn in ("cnf_rk4", "cnf_dopri5"):
        starts += [fn + ": y must be (BT,n,3)", fn + ": hyper has (3, 3080) rows for 2 frames", fn + ": the Hutchinson noise e and the initial",
                   fn + ": e (2, 129, 3) / logp (2, 128, 1) do not match y", fn + ": e (2, 128, 3) / logp (2, 128) do not match y",
                   fn + ": mbn_in must hold 12 floats", fn + ": mbn_out must hold 12 floats"]
    for fn in D.TRAIN:
        starts += [fn + ": y must be (BT,n,3)", fn + ": hyper must be (BT, >= 3078) rows and tcol hold 3078 floats, got (3, 3080)",
                   fn + ": hyper must be (BT, >= 3078) rows and tcol hold 3078 floats, got (2, 3077)",
                   fn + ": hyper must be (BT, >= 3078) rows and tcol hold 3078 floats, got (2, 3080) / (3077,)",
                   fn + ": the kernel is built for the 3-512-512-512-3 ODE function", fn + ": t_end must be a one-element device tensor"]
        starts.append(fn + (": the f16x3 weight packs w1h / w2h (ops.pack_cnf_h3) are required" if "_h3" in fn else
                            ": the bf16x6 weight packs w1x / w2x (ops.pack_cnf_x6) are required"))
        if "_h3" in fn:
            starts.append(fn + ": n = 127 is below the 128-point workgroup of the f16x3 kernel: %s is the wrapper for it" % fn.replace("_h3", ""))
        if fn in D.FRAMES:
            starts += [fn + ": max_steps must lie in 1..4096, got 0", fn + ": max_steps must lie in 1..4096, got 4097",
                       fn + ": ys must be a contiguous (4, 4, 2, 128, 3) tensor on cpu, got (5, 4, 2, 128, 3) on cpu",
                       fn + ": ka must be a contiguous (4, 4, 2, 128, 3) tensor on cpu, got (4, 4, 2, 129, 3) on cpu"]
    starts += ["cnf_train_fwd: e (2, 129, 3) / logp (2, 128, 1) do not match y", "cnf_train_fwd: e (2, 128, 3) / logp (2, 128) do not match y",
               "cnf_sample_tape_h3: steps must be positive", "caspr_amd.ops.CNF_TAPE_SPLIT must be 'bf16x6' or 'f16x3', got 'f16x4'"]
    for start in starts:
        assert any(t.startswith(start) for t in texts), start
    # every error is the one of the function that was called: a frame table's is cnf_rk4's, whoever asks (ops._chk_frame_table)
    for name, lines in GOLDEN.items():
        for line in lines:
            if line[0] == "raise" and ": " in line[2] and not line[2].startswith(("cnf_rk4: steps ", "cnf_rk4: order ", "caspr_amd.ops.")):
                assert line[2].split(":")[0] == name.split(":")[0], (name, line)


def test_both_positions_of_the_status_word_are_reached():
    behind = {}
    for line in FLAT:
        if "word" in line and line[0] in LAUNCHES:
            behind.setdefault(line[0], set()).add(line[line.index("word") - 1])
    assert set(behind) == {n for n in LAUNCHES if "_h3_" in n} and len(behind) == 5
    for name in ("caspr_cnf_rk4_h3_f32", "caspr_cnf_rk4_h3_frames_f32", "caspr_cnf_dopri5_h3_f32"):
        assert behind[name] == {"mbn_out", "null"}, name                  # ... t_end, [steps,] flags, mbn_in, mbn_out, word
    assert behind["caspr_cnf_sample_tape_h3_f32"] == {3}                    # ... t_end, steps, word
    assert behind["caspr_cnf_sample_tape_h3_frames_f32"] == {"order", "null"}        # ... t_end, steps, max_steps, order, word
    # the scope around every such launch: enter, the timer's first event, the launch, its second event, the post, leave
    for lines in GOLDEN.values():
        at = [i for i, line in enumerate(lines) if "word" in line and line[0] in LAUNCHES]
        for i in at:
            assert [line[:2] for line in lines[i - 1:i + 4:2]] == [["record", "ev0"], ["record", "ev1"], ["h3", "leave"]]
            assert lines[i + 2] == ["h3", "post", "word"] and ["h3", "enter"] in lines[:i - 1]


def test_both_spellings_of_the_narrow_flag_are_reached():
    plain = [line for line in FLAT if line[0] == "caspr_cnf_rk4_x6_f32"]
    # [name, the 13 arguments of the head, t_end, steps, flags, mbn_in, mbn_out, e, ...]
    assert {(line[HEAD + 2], line[HEAD + 5]) for line in plain} == {(0, "null"), (1, "null"), (2, "null"), (3, "null"), (0, "e"), (1, "e")}
    frames = [line for line in FLAT if line[0] == "caspr_cnf_rk4_x6_frames_f32"]
    assert {line[HEAD + 1] for line in frames} == {0, 1, 2, 3}             # [name, head, t_end, flags, ...]
    narrow_with_e = [n for n in GOLDEN if n.startswith("cnf_rk4") and "packs=x6:e=True:narrow=True" in n]
    assert len(narrow_with_e) >= 2 and all(GOLDEN[n][1][HEAD + 2] < 2 for n in narrow_with_e)


def test_the_hidden_width_each_front_end_passes():
    """ops.cnf_rk4 / cnf_dopri5 pass w0's rows and leave the 512 to C; the training wrappers check it and pass 512."""
    for fn in ("cnf_rk4", "cnf_dopri5"):
        line = [l for n, lines in GOLDEN.items() if n.startswith(fn) and n.endswith("bad=w0_shape") for l in lines if l[0] in LAUNCHES]
        assert len(line) == 1 and line[0][HEAD - 1] == 511
    assert {line[HEAD - 1] for line in FLAT if line[0].startswith(("caspr_cnf_sample_tape", "caspr_cnf_train_fwd"))} == {512}
    assert {line[3] for line in FLAT if line[0] in LAUNCHES} == {D.LDH}         # ldh: hyper's row stride
