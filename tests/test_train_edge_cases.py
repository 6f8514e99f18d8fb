"""The cases of tests/train_edge_cases.py, checked on the CPU (no GPU, no marker).

(a) Input conditions.  An f32 kernel and an f64 reference are comparable only away from discontinuities: every case whose backward
applies a ReLU mask keeps min |gamma xh + beta| >= 1e-3 over ALL elements (f64); every max without intended ties has a top-two gap
>= 1e-4 x the largest entry; the argmax_points cases are exact in f32, so their ties are exactly the planted ones.

(b) Controls that must fail.  For each kernel family a subtly wrong f64 variant of the reference is put through the comparison the
GPU tests use (test_hip_train.rel, the same bound) and must be rejected by at least 10 x the bound, or by an index mismatch.  A case
set that cannot tell one of these apart is too weak.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_hip_train
import train_edge_cases as E


@pytest.fixture(autouse=True)
def private_report(monkeypatch, tmp_path):
    """rel records every comparison in the GPU suite's parity report: the controls go to a private one."""
    monkeypatch.setattr(test_hip_train, "REPORT", {})
    monkeypatch.setattr(test_hip_train, "ROOT", str(tmp_path))


def accepted(got, want, bound, ref=None):
    test_hip_train.rel("control", got, want, bound, ref=ref)


def rejected(got, want, bound, ref=None):
    """The comparison of the GPU tests refuses `got` even at 10 x its bound."""
    with pytest.raises(AssertionError):
        test_hip_train.rel("control", got, want, 10.0 * bound, ref=ref)


# ---------------------------------------------------------------------------------------------
# (a) input conditions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,C", E.GN_BWD_SHAPES)
def test_gn_bwd_cases_keep_clear_of_the_relu_and_plant_the_max(B, P, C):
    c = E.case_gn_bwd(B, P, C)
    assert E.relu_margin(c.pre) >= E.RELU_MARGIN
    if P >= 5:
        assert 0.3 <= float((c.pre > 0).double().mean()) <= 0.7, "about half of the elements rectified"
    assert E.max_gap_ok(c.pre)
    rows = set(c.amax.flatten().tolist())
    assert rows == {P - 1, 0, P // 2}, "the max over points sits in the last row (the last split), in row 0 and in the middle"
    for k in ("dY", "dgamma", "dbeta"):        # the closed form the controls are built from IS the reference
        accepted(E.gn_bwd_formula(c, True)[k], E.gn_bwd_want(c, True, False, True)[k], 1e-12)


@pytest.mark.parametrize("C", E.ROWS_C)
def test_gn_rows_small_cases_meet_their_conditions(C):
    for ns in E.ROWS_NS:
        for NB in E.ROWS_NB:
            for relu in (False, True):
                c = E.small_rows_case(1, NB, ns, C, relu)        # raises when no seed in 0..19 passes
                assert E.rows_case_ok(c)
                if relu and ns * C >= 256:
                    assert 0.25 <= float((c.pre > 0).double().mean()) <= 0.75


@pytest.mark.parametrize("C,ns,dup", E.ROWS_DUP)
def test_gn_rows_repeated_rows_are_exact_ties(C, ns, dup):
    for relu in (False, True):
        c = E.small_rows_case(1, 5, ns, C, relu, dup)
        assert E.rows_case_ok(c)
        y = c.y.reshape(5, ns, C)
        rep, src = E.repeated_rows(ns, dup), E.source_row(ns, dup)
        assert torch.equal(y[:, rep], y[:, src:src + 1].expand(5, len(rep), C))
        assert not bool(torch.isin(c.want["arg"], torch.tensor(rep, dtype=torch.int32)).any()), "first occurrence: never a repeated row"
        hit0 = c.want["arg"] == src
        assert bool(hit0.any()) and bool(hit0.all()) == (len(rep) == ns - 1), "the repeated row wins in some columns, in all when every row repeats it"
        A = F.relu(c.pre) if relu else c.pre
        assert bool(((A.gather(1, c.want["arg"].long().unsqueeze(1)).squeeze(1) > 0) & hit0).any()), "and carries a gradient there"


@pytest.mark.parametrize("direction,C,ns", [("fwd", 16, 2), ("bwd", 16, 2), ("bwd", 512, 1)])
def test_gn_rows_grid_stride_cases_meet_their_conditions(direction, C, ns):
    c = E.stride_rows_case(direction, C, ns)
    assert E.rows_case_ok(c) and E.relu_margin(c.pre) >= 10 * E.RELU_MARGIN
    assert c.NB == (E.ROWS_FWD_STRIDE if direction == "fwd" else E.ROWS_BWD_STRIDE)
    assert c.NB > 4 * (8192 if direction == "fwd" else 2048), "more neighbourhoods than the capped grid has waves"
    assert 0.25 <= float((c.pre > 0).double().mean()) <= 0.75


@pytest.mark.parametrize("B,P,C,pairs", E.ARGMAX_CASES)
def test_argmax_cases_are_exact_and_tie_only_where_planted(B, P, C, pairs):
    c = E.case_argmax(B, P, C, pairs)
    assert float(c.y.abs().max()) <= 64 and torch.equal(c.y, c.y.round())
    m, e = np.frexp(c.scale.numpy())
    assert bool(((np.abs(m) == 0.5) | (m == 0)).all()), "scale: +- a power of two, or 0"
    v32 = c.y * c.scale.unsqueeze(1) + c.shift.unsqueeze(1)
    assert torch.equal(v32.double(), c.v), "y scale + shift is exact in f32"
    at_max = (c.v == c.v.max(dim=1, keepdim=True).values).sum(dim=1).numpy()
    zero = c.scale.numpy() == 0
    assert (at_max[zero] == P).all() and (c.want.numpy()[zero] == 0).all()
    assert (at_max[~zero & c.planted] == 2).all() and (at_max[~zero & ~c.planted] == 1).all()
    if pairs:
        where = torch.from_numpy(c.planted)
        assert c.planted.any() and (C == 1 or (bool((c.scale[where] < 0).any()) and bool((c.scale[where] > 0).any())))
        for b, col in zip(*np.nonzero(c.planted)):
            assert int(c.want[b, col]) == min(pairs[(col + b) % (len(pairs) + 1)])


@pytest.mark.parametrize("B,P,C,groups", E.GN_STATS_CASES)
def test_gn_stats_cases(B, P, C, groups):
    c = E.case_gn_stats(B, P, C, groups)
    assert float(c.gamma[0]) == 0.0 and int((c.gamma < 0).sum()) >= 2
    assert abs(float(c.want["mean"][B - 1].mean()) - 1000.0) < 1.0 and abs(float(c.want["mean"][0].mean())) < 1.0
    # scale / shift are the affine form of group_norm: y scale + shift reproduces it
    a = E.gn_pre(c.y.double(), c.gamma.double(), c.beta.double(), groups)
    accepted(c.y.double() * c.want["scale"].unsqueeze(1) + c.want["shift"].unsqueeze(1), a, 1e-9)
    # the affine form in plain f32 keeps pmax to ~1e-7 except on the entry around 1000: only that tensor's bound is raised, to twice
    # the f32 figure and never above 2e-4
    for b in range(B - 1):
        assert E.pmax_f32_error(c, b) <= 0.1 * E.ENC_FWD
    assert 0.5 * E.ENC_FWD <= E.pmax_f32_error(c, B - 1) <= 2e-4
    assert E.ENC_FWD <= E.pmax_bound(c, B - 1) <= min(2e-4, 4 * E.pmax_f32_error(c, B - 1))


# ---------------------------------------------------------------------------------------------
# (b) controls that must fail
# ---------------------------------------------------------------------------------------------
def test_control_tie_broken_to_the_last_index():
    for B, P, C, pairs in E.ARGMAX_CASES:
        good, bad = E.case_argmax(B, P, C, pairs), E.case_argmax(B, P, C, pairs, last=True)
        assert torch.equal(good.y, bad.y)
        assert torch.equal(good.want, bad.want) == (P == 1), "argmax_points: last-index ties go unnoticed at %s" % ((B, P, C, pairs),)
    for C, ns, dup in E.ROWS_DUP:
        c = E.small_rows_case(1, 5, ns, C, True, dup)
        A = F.relu(c.pre).numpy()
        last = ns - 1 - np.argmax(A[:, ::-1], axis=1)
        assert not np.array_equal(last, c.want["arg"].numpy()), "gn_rows: last-index ties go unnoticed"
        # and the gradient routed to the last of the equal rows is refused by the dY comparison
        y6 = c.y.double().reshape(c.NB, ns, C).requires_grad_(True)
        a = F.relu(E.rows_pre(y6, c.gamma.double(), c.beta.double(), c.eps))
        (a.gather(1, torch.from_numpy(last).unsqueeze(1)).squeeze(1) * c.dmax.double().reshape(c.NB, C)).sum().backward()
        rejected(y6.grad.reshape(1, c.NB * ns, C), c.want["dmax"]["dY"], E.ROWS_GRAD)


def test_control_relu_mask_shifted_by_one_row():
    """No case plants exact zeros in front of the ReLU (they would sit ON the discontinuity), so the control shifts the mask."""
    for B, P, C in E.GN_BWD_SHAPES:
        if P == 1:
            continue
        c = E.case_gn_bwd(B, P, C)
        want = E.gn_bwd_want(c, True, False, True)
        bad = E.gn_bwd_formula(c, True, mask_shift=1)
        rejected(bad["dY"], want["dY"], E.GN_GRAD)
        rejected(bad["dbeta"], want["dbeta"], E.GN_GRAD)
    c = E.small_rows_case(1, 5, 5, 64, True)
    y6 = c.y.double().reshape(5, 5, 64).requires_grad_(True)
    pre = E.rows_pre(y6, c.gamma.double(), c.beta.double(), c.eps)
    ((pre * torch.roll(c.pre > 0, 1, dims=1)) * c.da.double().reshape(5, 5, 64)).sum().backward()
    rejected(y6.grad.reshape(1, 25, 64), c.want["dense"]["dY"], E.ROWS_GRAD)


def test_control_gn_bwd_mean_term_over_points_only():
    for B, P, C in E.GN_BWD_SHAPES:
        c = E.case_gn_bwd(B, P, C)
        rejected(E.gn_bwd_formula(c, True, n=P)["dY"], E.gn_bwd_want(c, True, False, True)["dY"], E.GN_GRAD)


def test_control_split_boundary_row_dropped():
    # gn_stats: row 1024, the first of the second 1024-row split
    for B, P, C, groups in [(3, 1025, 64, 16), (3, 2049, 64, 16), (3, 1025, 192, 16), (3, 1025, 16, 4)]:
        good, bad = E.case_gn_stats(B, P, C, groups), E.case_gn_stats(B, P, C, groups, drop_row=1024)
        for b in range(B - 1):          # per batch entry, as the GPU test compares them: the entry around 1000 would hide the others
            for k in ("shift", "mean", "rstd"):
                rejected(bad.want[k][b], good.want[k][b], E.ENC_FWD)
    # gn_bwd: the same row out of dgamma / dbeta
    for B, P, C in [(3, 1025, 64), (2, 1030, 192), (3, 2049, 128)]:
        c = E.case_gn_bwd(B, P, C)
        want, bad = E.gn_bwd_want(c, True, False, True), E.gn_bwd_formula(c, True, drop_row=1024)
        rejected(bad["dgamma"], want["dgamma"], E.GN_GRAD)
        rejected(bad["dbeta"], want["dbeta"], E.GN_GRAD)
    # colsum_batched: row 512
    for C in E.COLSUM_C:
        for P in (513, 1030):
            rejected(E.case_colsum(3, P, C, drop_row=512).want, E.case_colsum(3, P, C).want, E.COLSUM)
    # the CNF layers: the first point of the second of eight splits
    for C, n in [(132, 256), (512, 257), (132, 300), (4, 257)]:
        c = E.case_cnf_act(3, n, C)
        per = (n + 7) // 8
        assert E.value_splits(n) == 8
        good, bad = E.cnf_dgate_formula(c), E.cnf_dgate_formula(c, drop_point=per)
        for k in ("dgate", "dbeta"):
            accepted(good[k], c.want["dh"][k], 1e-9)
            rejected(bad[k], c.want["dh"][k], E.GRAD)
    # the skinny weight gradient: its last row
    for B, P, Cin, Cout in E.WGRAD_SKINNY:
        rejected(E.case_wgrad_skinny(B, P, Cin, Cout, drop_row=B * P - 1).want, E.case_wgrad_skinny(B, P, Cin, Cout).want, E.WGRAD)


def test_control_last_neighbourhood_of_a_grid_stride_pass_dropped():
    for C, ns in ((16, 2), (512, 1)):
        c = E.stride_rows_case("bwd", C, ns)
        for mode in ("dense", "dmax"):
            y6, ga6, be6 = (t.double().requires_grad_(True) for t in (c.y.reshape(c.NB, ns, C)[:-1], c.gamma, c.beta))
            A = F.relu(E.rows_pre(y6, ga6, be6, c.eps))
            if mode == "dense":
                loss = (A * c.da.double().reshape(c.NB, ns, C)[:-1]).sum()
            else:
                loss = (A.gather(1, c.want["arg"].long()[:-1].unsqueeze(1)).squeeze(1) * c.dmax.double().reshape(c.NB, C)[:-1]).sum()
            loss.backward()
            rejected(ga6.grad, c.want[mode]["dgamma"], E.ROWS_GRAD)
            rejected(be6.grad, c.want[mode]["dbeta"], E.ROWS_GRAD)
    f = E.stride_rows_case("fwd")
    assert not torch.equal(f.want["arg"][-1], f.want["arg"][-2]), "the forward pass: a stale last neighbourhood shows in arg"
    assert not torch.equal(f.want["A"][0, -2:] > 0, f.want["A"][0, -4:-2] > 0)


def test_control_padding_column_read_as_data():
    """The pad columns of every input hold NaN: a kernel that reads one returns a non-finite value, which rel refuses.  With a finite
    pad the comparisons still notice (here: the pad taken as channel C - 1 of the column sums, as the fifth output of a weight gradient)."""
    for C in E.COLSUM_C:
        c = E.case_colsum(3, 513, C)
        buf = E.embed(c.a)
        shifted = buf[:, :, 1:C + 1].double().sum(dim=1)
        with pytest.raises(AssertionError, match="non-finite"):
            test_hip_train.rel("control", shifted, c.want, 1.0)
        rejected(E.embed(c.a, fill=1.0)[:, :, 1:C + 1].double().sum(dim=1), c.want, E.COLSUM)
    c = E.case_wgrad_skinny(2, 1027, 260, 1)
    dy = c.dy.clone()
    dy[:, :, 1] = 1.0                              # a dirty column past Cout lands in the row below of the (Cout, Cin) result
    assert float(dy.double()[:, :, 1].abs().sum()) > 0
    leaked = torch.einsum("bpo,bpi->oi", dy.double()[:, :, :2], c.x.double()).sum(dim=0, keepdim=True)
    rejected(leaked, c.want, E.WGRAD)


def test_control_pmax_takes_the_max_under_a_negative_scale():
    for B, P, C, groups in E.GN_STATS_CASES:
        if P == 1:
            continue                               # one point: max and min coincide
        good, bad = E.case_gn_stats(B, P, C, groups), E.case_gn_stats(B, P, C, groups, pmax_rule="max under negative scale")
        neg = good.gamma < 0
        accepted(bad.want["pmax"][:, ~neg], good.want["pmax"][:, ~neg], 1e-9)
        rejected(bad.want["pmax"], good.want["pmax"], E.ENC_FWD)
    # the affine form with the right rule IS the reference
    good, aff = E.case_gn_stats(3, 1025, 64), E.case_gn_stats(3, 1025, 64, pmax_rule="affine")
    accepted(aff.want["pmax"], good.want["pmax"], 1e-9)


def test_control_in_relu_from_off_by_a_quad():
    for B, P, Cin, Cout, frm in E.WGRAD_RELU_FROM:
        good = E.case_wgrad_relu_from(B, P, Cin, Cout, frm)
        if frm < Cin:
            rejected(E.case_wgrad_relu_from(B, P, Cin, Cout, frm, ref_from=frm + 4).want["dW"], good.want["dW"], E.WGRAD)
        rejected(E.case_wgrad_relu_from(B, P, Cin, Cout, frm, ref_from=frm - 4).want["dW"], good.want["dW"], E.WGRAD)


def test_control_gate_of_frame_0_for_all_frames():
    for C, n in E.CNF_GRID:
        good, bad = E.case_cnf_in(3, n, C), E.case_cnf_in(3, n, C, gate_frame0=True)
        rejected(bad.want["h"], good.want["h"], E.FWD)
        rejected(bad.want["dy"], good.want["dy"], E.GRAD)


def test_control_dgate_summed_without_the_bias():
    for C, n in E.CNF_GRID:
        c = E.case_cnf_act(3, n, C)
        accepted(E.cnf_dgate_formula(c)["dgate"], c.want["dh"]["dgate"], 1e-9)
        rejected(E.cnf_dgate_formula(c, with_b=False)["dgate"], c.want["dh"]["dgate"], E.GRAD)


def test_cnf_act_cases_reach_the_tails():
    c = E.case_cnf_act(3, 257, 132)
    a = (c.z.double() + c.b.double()) * c.gate.double().repeat_interleave(257, 0) + c.beta.double().repeat_interleave(257, 0)
    assert float(a.max()) > 20 and float(a.min()) < -20, "pre-activations far into both tails of softplus / sigmoid"
    assert E.value_splits(255) == 1 and E.value_splits(256) == 8
