"""The pointwise conv front-end of caspr_amd/ops.py as a dispatch, on the CPU: which entry each call reaches, with which arguments in
which order, and the event and stream order of the two side-stream functions, against the transcript the front-end gave before it was
rewritten around one route table (tests/golden/conv_dispatch_parent.json; conv_dispatch_cases.py says how it was made)."""
import os

import pytest

import conv_dispatch_cases as D
from caspr_amd import lib

GOLDEN = D.load(os.path.join(os.path.dirname(__file__), "golden", "conv_dispatch_parent.json"))


def test_the_golden_file_is_the_case_table():
    assert list(GOLDEN) == [c.name for c in D.CASES]
    assert 100 <= len(D.CASES) <= 400


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_transcript(name):
    got = D.transcript(D.BY_NAME[name])
    assert "unknown" not in [v for line in got for v in line], "a pointer that belongs to no tensor of the call"
    assert got == GOLDEN[name]


def test_every_entry_of_the_front_end_is_reached():
    """Every forward conv entry and every GroupNorm-statistics entry of lib.SIGNATURES, but the fused conv + activation of the CNF training
    tier (train/flow_grad.py launches it, not this front-end)."""
    want = {n for n in lib.SIGNATURES if (n.startswith("caspr_conv1x1_") and "wgrad" not in n and "bwd" not in n and "cnf_act" not in n)
            or n.startswith("caspr_conv_gn_") or n.startswith("caspr_gn_stats")}
    assert len(want) >= 14
    seen = {line[0] for lines in GOLDEN.values() for line in lines}
    assert want <= seen, sorted(want - seen)


def test_every_error_of_the_front_end_is_reached():
    texts = [line[2] for lines in GOLDEN.values() for line in lines if line[0] == "raise"]
    for start in ("conv1x1: input rows hold", "conv1x1_gn: input rows hold", "conv1x1_gn: pool=3 must divide the 4 batch entries",
                  "conv1x1_gn: pool=0 must divide", "conv1x1_gn_early: this layer does not run",
                  "caspr_amd.ops.CONV_SPLIT must be 'bf16x6' or 'f16x3', got 'f16x4'"):
        assert any(t.startswith(start) for t in texts), start


def test_every_route_and_every_branch_of_the_side_streams_is_reached():
    flat = [line for lines in GOLDEN.values() for line in lines]
    assert any(line[:2] == ["wait_stream", "tail"] for line in flat) and any(line[0] == "on_early" for line in flat)
    assert any(line[0] == "record_stream" and line[1] == "bias" for line in flat)
    # conv1x1_gn_early: the remainder on the tail stream, and behind the main tiles (with_tail = 1 on the launch of tiles [1, 3))
    part = [line for line in flat if line[0].endswith("_part_f32")]
    # [name, main, tail, the 14 arguments of the head, mt0, mt1, with_tail, reserve, ...]; the form is the name's third word
    tiles = {(line[0].split("_")[2],) + tuple(line[17:21]) for line in part}
    assert {t[0] for t in tiles} == {"x6w", "h3w"}
    for form in ("x6w", "h3w"):
        assert {(form, 0, 1, 0, 0), (form, 3, 3, 1, 0), (form, 1, 3, 0, 32), (form, 1, 3, 1, 32), (form, 1, 3, 1, 0), (form, 0, 3, 0, 0)} <= tiles
