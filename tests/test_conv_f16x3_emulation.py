"""The f16x3 conv contract (tests/conv_f16x3_ref.py) on the CPU: against the f64 contraction on the inputs of
test_hip_parity.test_conv1x1_x6w_kernel at that test's tolerance, and inside the f64 oracle's encoder at the pipeline's flat 1e-5.

In the encoder the restatement replaces the matrix product of every layer the host's rule (conv_f16x3_ref.routed: >= 512 input and
output channels, >= 1024 rows per batch entry, a multiple of 128) sends to the persistent 512-channel kernel -- the first
cout - cout % 512 output channels of it, the remainder stays exact, as it stays on bf16x6 -- and nothing else: activations enter it
rounded to f32, as the kernel reads them, everything around it stays f64.  The rule is applied to the oracle's own layer shapes; for
encoder.conv1 to the 576 columns the host's layer multiplies (the tiled global feature enters as a per-batch bias, exactly)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_f16x3_ref as R
from oracle import model as O
from caspr_amd.utils.synthetic import car_sequences

SHAPES = [(1, 1280, 1600, 1600), (2, 256, 512, 512), (1, 384, 1536, 512), (1, 128, 256, 1088), (3, 128, 512, 560)]
PIPELINE_BOUND = 1e-5


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).normal(0, 1, shape) * scale).astype(np.float32))


@pytest.mark.parametrize("B,P_,Cin,Cout", SHAPES)
def test_three_f16_products_conv_matches_f64(B, P_, Cin, Cout):
    """The operands of test_conv1x1_x6w_kernel, fused and plain.  Channels past the last full 512 are multiplied in f32 (they stay on
    the bf16x6 tail kernel).  The first-product-only control must miss the tolerance, so that the test is able to fail."""
    w = rnd(1, Cout, Cin, scale=1.0 / np.sqrt(Cin))
    b, bb = rnd(2, Cout, scale=0.3), rnd(3, B, Cout, scale=0.1)
    x = rnd(Cin + Cout, B, P_, Cin)
    sc_in, sh_in = rnd(4, B, Cin).abs() + 0.5, rnd(5, B, Cin)
    cm = Cout - Cout % 512
    for fused in (True, False):
        kw = dict(in_scale=sc_in, in_shift=sh_in, in_relu=True, in_relu_from=8) if fused else {}
        xin = R.transform(x, **kw)
        y64 = xin.double() @ w.double().t() + b.double() + (bb.double().unsqueeze(1) if fused else 0.0)
        tol = 2e-6 * max(1.0, float(y64.abs().max()))
        errs = []
        for first_only in (False, True):
            y, bad = R.conv(x, w[:cm], b[:cm], bb[:, :cm] if fused else None, first_only=first_only, **kw)
            assert not bool(bad.any())
            rest = xin @ w[cm:].t() + b[cm:] + (bb[:, cm:].unsqueeze(1) if fused else 0.0)
            errs.append(float((torch.cat([y, rest], dim=2).double() - y64).abs().max()))
        print("f16x3 conv emulation %dx%d %s: max |y - y_f64| = %.3e (tolerance %.3e), first product only %.3e"
              % (Cin, Cout, "fused" if fused else "plain", errs[0], tol, errs[1]))
        assert errs[0] <= tol, (errs[0], tol)
        assert errs[1] > tol, (errs[1], tol)


def test_range_rule():
    x = torch.zeros(1, 4, 32)
    x[0, 1, 3], x[0, 2, 5], x[0, 3, 7] = 4095.0, float("nan"), -4094.9
    y, bad = R.conv(x, torch.ones(512, 32))
    assert bad.tolist() == [[False, True, True, False]]
    assert bool(torch.isnan(y[0, 1]).all()) and bool(torch.isnan(y[0, 2]).all()) and bool(torch.isfinite(y[0, 0]).all()) and bool(torch.isfinite(y[0, 3]).all())
    assert float((y[0, 3] + 4094.9).abs().max()) < 1e-3


class _Routed:
    """oracle.model._conv with the routed layers' products on the restatement."""

    def __init__(self, first_only=False):
        self.first_only, self.layers = first_only, []

    def __call__(self, sd, key, x):
        w, b = sd[key + ".weight"], sd[key + ".bias"]
        cout, cin, rows = w.shape[0], w.shape[1], x.shape[2]
        cols = torch.arange(cin)
        if key == "encoder.conv1":             # [local 512 | tiled global 1024 | point feature 64]: the host's layer multiplies local + point feature
            cols = torch.cat([cols[:512], cols[1536:]])
        if x.dtype != torch.float64 or not R.routed(len(cols), cout, rows):
            return F.conv1d(x, w, b)
        cm = cout - cout % 512
        self.layers.append((key, len(cols), cout, rows))
        y = F.conv1d(x, w, b)                                                       # f64: the remainder channels and the other columns
        w2 = w[:cm, :, 0]
        other = torch.ones(cin, dtype=torch.bool)
        other[cols] = False
        part, bad = R.conv(x[:, cols].transpose(1, 2).float(), w2[:, cols].float(), first_only=self.first_only)
        assert not bool(bad.any())
        exact_rest = torch.einsum("oc,bcp->bop", w2[:, other], x[:, other]) + b[:cm].view(1, -1, 1)
        y[:, :cm] = part.transpose(1, 2).double() + exact_rest
        return y


def test_encoder_with_routed_layers_on_three_f16_products(seeded_sd, monkeypatch):
    """z0 and T-NOCS of the f64 encoder with the routed layers on the restatement, against the pure f64 encoder, at the smallest
    sequence the oracle tests use (1 x 2 frames x 1024 points).  Measured: see DESIGN.md section 3 (the figures are printed)."""
    sd64 = {k: v.double() for k, v in seeded_sd.items()}
    x, _ = car_sequences(1, 2, 1024, seed=1234)
    z64, t64 = O.encode(sd64, x.double())
    sub = _Routed()
    monkeypatch.setattr(O, "_conv", sub)
    z, t = O.encode(sd64, x.double())
    assert len(sub.layers) >= 2 and any(k == "encoder.conv2" for k, _, _, _ in sub.layers), sub.layers
    ez, et = float((z - z64).abs().max()), float((t - t64).abs().max())
    ctl = _Routed(first_only=True)
    monkeypatch.setattr(O, "_conv", ctl)
    zc, tc = O.encode(sd64, x.double())
    cz, ct = float((zc - z64).abs().max()), float((tc - t64).abs().max())
    print("f16x3 conv inside the f64 encoder: layers %s\n  max |z0 - z0_f64| = %.3e, |tnocs - tnocs_f64| = %.3e (bound %.1e); first product only %.3e / %.3e"
          % (sub.layers, ez, et, PIPELINE_BOUND, cz, ct))
    assert ez <= PIPELINE_BOUND and et <= PIPELINE_BOUND, (ez, et)
    assert max(cz, ct) > PIPELINE_BOUND, (cz, ct)
