"""CPU restatement (torch, no GPU) of the arithmetic contract of the f16x3 point-CNF kernel (csrc/ode_f16x3w.hip): an f32 matrix
product on three f16 products.

    a . b  ~  a1 b1 + a1 b2 + a2 b1          a = a1 + a2 (+ a3, dropped), both planes f16, round to nearest even

 * exact power-of-two prescales keep both planes inside f16's exponent range: activations x 2^4 (ACT_SHIFT), a layer's weights x 2^s
   with s the integer that puts max |W| in [2^14, 2^15) (weight_shift);
 * a plane value below 2^-14 in magnitude -- an f16 subnormal -- is flushed to zero EXPLICITLY, as the kernel does, so nothing here
   depends on whether the matrix pipe honours f16 subnormals;
 * the three products accumulate in f32 and the result is unscaled by 2^-(4 + s), exactly.

split() is the contract of one operand side; linear() is a drop-in for torch.nn.functional.linear on a (512, 512) hidden layer."""
import math

import torch

ACT_SHIFT = 4
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0
F32_MIN_NORMAL = 2.0 ** -126
MAX_SHIFT = 100


def weight_shift(w):
    """s with max |w| * 2^s in [2^14, 2^15); 0 for an all-zero, subnormal or non-finite layer; at most MAX_SHIFT (the kernel's
    XH_MAX_SHIFT: the unscale factor 2^-(4 + s) stays a normal f32 number; it binds only where max |w| < 2^-86)."""
    m = float(w.detach().float().abs().max())
    if m < F32_MIN_NORMAL or not math.isfinite(m):
        return 0
    return min(14 - math.frexp(m)[1] + 1, MAX_SHIFT)          # frexp: m = f * 2^e with f in [0.5, 1)  ->  floor(log2 m) = e - 1


def _flush(p):
    return torch.where(p.abs() < F16_MIN_NORMAL, torch.zeros_like(p), p)


def split(x):
    """f32 x (already prescaled) -> (p1, p2) as f32 tensors holding f16 values: p1 = rne16(x), p2 = rne16(x - p1), subnormal plane
    values flushed.  |x| must be below 65520 (the kernel's range guard): rne16 would give inf."""
    x = x.float()
    p1 = _flush(x.half().float())
    p2 = _flush((x - p1).half().float())
    return p1, p2


def linear(x, w, b=None, first_only=False):
    """x (..., K) f32, w (M, K) f32 -> x w^T (+ b) on three f16 products with f32 accumulation.  first_only: a1 b1 alone (the
    control that shows what the two cross terms buy)."""
    s = weight_shift(w)
    a1, a2 = split(x.float() * 2.0 ** ACT_SHIFT)
    w1, w2 = split(w.float() * 2.0 ** s)
    if first_only:
        acc = a1 @ w1.T
    else:
        acc = a2 @ w1.T           # smallest terms first, as the kernel orders them
        acc = acc + a1 @ w2.T
        acc = acc + a1 @ w1.T
    out = acc * 2.0 ** -(ACT_SHIFT + s)
    return out if b is None else out + b
