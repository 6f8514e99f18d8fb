"""CPU restatement (torch, no GPU) of the arithmetic contract of the f16x3 pointwise conv (csrc/gemm_f16x3w.hip): the 512-channel tiles
of a wide layer on three f16 products per f32 product.  The split of one operand side is tests/f16x3_ref.py's (left as it is).

    x  ->  v = relu_from(fma(x, scale, shift))            the producer's GroupNorm scale / shift, the ReLU from channel in_relu_from on
       ->  V = 16 v                                       exact; a V that is not below 65520 in magnitude (NaN, infinity included) is the
                                                          range guard's: hi plane NaN, lo plane 0 -> the row's outputs are NaN
       ->  (V1, V2) = split(V)                            SIGNED: both planes flushed by magnitude below 2^-14
    W  ->  (W1, W2) = split(W 2^s), s = weight_shift(W)   per layer, over the rows the kernel takes
    y   =  (W2 V1 + W1 V2 + W1 V1) 2^-(4 + s) + bias + per-batch bias        f32 accumulation, smallest terms first, exact unscale
"""
import torch

from f16x3_ref import ACT_SHIFT, split, weight_shift

F16_LIMIT = 65520.0        # the smallest f32 that rounds to infinity in f16


def transform(x, in_scale=None, in_shift=None, in_relu=False, in_relu_from=0):
    """x (B, P, Cin) f32 -> the conv's operand: one fused multiply-add per value (one rounding), then the ReLU from in_relu_from on."""
    v = x.float()
    if in_scale is not None:
        v = (v.double() * in_scale.double().unsqueeze(1) + in_shift.double().unsqueeze(1)).float()      # the product is exact in f64
        if in_relu:
            v = torch.cat([v[..., :in_relu_from], torch.relu(v[..., in_relu_from:])], dim=-1)
    return v


def conv(x, w, bias=None, bbias=None, in_scale=None, in_shift=None, in_relu=False, in_relu_from=0, first_only=False):
    """x (B, P, Cin) f32, w (Cout, Cin) f32 -> (y (B, P, Cout) f32, tripped (B, P) bool: the rows the range guard turns into NaN).
    first_only: W1 V1 alone (the control that shows what the two cross terms buy)."""
    V = transform(x, in_scale, in_shift, in_relu, in_relu_from) * 2.0 ** ACT_SHIFT
    bad = ~(V.abs() < F16_LIMIT)
    V1, V2 = split(torch.where(bad, torch.zeros_like(V), V))
    V1 = torch.where(bad, torch.full_like(V1, float("nan")), V1)
    s = weight_shift(w)
    W1, W2 = split(w.float() * 2.0 ** s)
    if first_only:
        acc = V1 @ W1.T
    else:
        acc = V1 @ W2.T
        acc = acc + V2 @ W1.T
        acc = acc + V1 @ W1.T
    y = acc * 2.0 ** -(ACT_SHIFT + s)
    if bias is not None:
        y = y + bias
    if bbias is not None:
        y = y + bbias.unsqueeze(1)
    return y, bad.any(dim=-1)


def routed(cin, cout, rows, min_cin=512, min_rows=1024):
    """The rule of caspr_amd.ops for the persistent 512-channel kernel: the layers it takes, and with conv_split = "f16x3" the new
    kernel takes the first cout - cout % 512 channels of them."""
    return cin % 32 == 0 and cin >= min_cin and cout >= 512 and cout % 4 == 0 and rows >= min_rows and rows % 128 == 0
