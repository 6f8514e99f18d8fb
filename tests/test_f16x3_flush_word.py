"""The flush of f16-subnormal plane values ON THE f16 WORD (csrc/f16x3_common.h: xh_flush_word, used by csrc/ode_f16x3w.hip), restated
with numpy on the CPU and held against the contract tests/f16x3_ref.py: split(), and against the form the kernel had before (compare the
f32 value with XH_FLUSH = 2^-14 - 2^-25 and select 0 in front of the conversion).

    new:  h1 = zero_exp0(rne16(x));  r = x - h1;  h2 = zero_exp0(rne16(r))        zero_exp0(h) = h * min(e(h), 1) per half,
    old:  a = x < F ? 0 : x;  h1 = rne16(a);  r = a - h1;  h2 = rne16(|r| < F ? 0 : r)       e(h) = (h [& 0x7fff]) >> 10

Both plane WORDS must be equal -- on every f32 in [2^-17, 2^-12) of both signs (the threshold with three binades below and two above
it), on first planes in 2^-2 .. 2^0 whose remainder sweeps that band, and on the specials.  numpy's f32 -> f16 conversion rounds to
nearest even, as v_cvt_pk_f16_f32 does."""
import numpy as np
import pytest
import torch

import f16x3_ref as R

XH_FLUSH = np.float32(2.0 ** -14 - 2.0 ** -25)


def rne16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(np.float16).view(np.uint16)


def zero_exp0(h, signed):
    """xh_flush_word on one half: v_pk_lshrrev_b16 / v_pk_min_u16 / v_pk_mul_lo_u16 (and the v_and_b32 of the signed form)."""
    e = ((h & np.uint16(0x7fff)) if signed else h) >> np.uint16(10)
    return (h * np.minimum(e, np.uint16(1))).astype(np.uint16)


def split_new(x, signed1):
    h1 = zero_exp0(rne16(x), signed1)
    with np.errstate(invalid="ignore"):
        r = x - h1.view(np.float16).astype(np.float32)
    return h1, zero_exp0(rne16(r), True)


def split_old(x):
    """The kernel's earlier form; plane 1 as it was written for X >= 0 (x < F), plane 2 on |r|."""
    a = np.where(x < XH_FLUSH, np.float32(0), x)
    h1 = rne16(a)
    with np.errstate(invalid="ignore"):
        r = a - h1.view(np.float16).astype(np.float32)
    return h1, rne16(np.where(np.abs(r) < XH_FLUSH, np.float32(0), r))


def split_ref(x):
    p1, p2 = R.split(torch.from_numpy(x))
    return p1.half().view(torch.int16).numpy().view(np.uint16), p2.half().view(torch.int16).numpy().view(np.uint16)


def same_words(got, want, what):
    nan_g, nan_w = (got & 0x7fff) > 0x7c00, (want & 0x7fff) > 0x7c00          # NaN: any payload
    bad = (nan_g != nan_w) | (~nan_g & (got != want))
    assert not bad.any(), "%s: %d of %d words differ, first at index %d: %#06x vs %#06x" % (
        what, int(bad.sum()), bad.size, int(np.argmax(bad)), int(got[np.argmax(bad)]), int(want[np.argmax(bad)]))


@pytest.mark.parametrize("binade", range(-17, -12))
def test_every_f32_around_the_threshold(binade):
    """All 2^23 f32 values of one binade of [2^-17, 2^-12), both signs."""
    x = (np.arange(1 << 23, dtype=np.uint32) + np.uint32((127 + binade) << 23)).view(np.float32)
    assert x[0] == np.float32(2.0 ** binade) and x[-1] < np.float32(2.0 ** (binade + 1))
    r1, r2 = split_ref(x)
    for signed1 in (False, True):          # the kernel's first plane has X >= 0 and leaves the sign in e; the contract is symmetric
        h1, h2 = split_new(x, signed1)
        same_words(h1, r1, "plane 1 of 2^%d (signed %s)" % (binade, signed1))
        same_words(h2, r2, "plane 2 of 2^%d (signed %s)" % (binade, signed1))
    o1, o2 = split_old(x)
    same_words(h1, o1, "plane 1 of 2^%d against the compare-and-select form" % binade)
    same_words(h2, o2, "plane 2 of 2^%d against the compare-and-select form" % binade)
    n1, n2 = split_new(-x, True)
    m1, m2 = split_ref(-x)
    same_words(n1, m1, "plane 1 of -2^%d" % binade)
    same_words(n2, m2, "plane 2 of -2^%d" % binade)
    assert (n2 != 0x8000).all() and (h2 != 0x8000).all(), "a flushed remainder is +0, whatever its sign"


@pytest.mark.parametrize("base", (0.25, 0.5, 0.999))
def test_remainders_in_the_band(base):
    """First planes that are ordinary f16 numbers (ulp 2^-12 or 2^-11) with remainders of both signs from 2^-17 up to half an ulp: the second
    plane's flush decides around +-2^-14."""
    r = (np.arange(0, 5 << 23, 61, dtype=np.uint32) + np.uint32((127 - 17) << 23)).view(np.float32)
    for sgn in (1.0, -1.0):
        x = (np.float32(base) + np.float32(sgn) * r).astype(np.float32)
        h1, h2 = split_new(x, False)
        r1, r2 = split_ref(x)
        o1, o2 = split_old(x)
        same_words(h1, r1, "plane 1")
        same_words(h2, r2, "plane 2")
        same_words(h1, o1, "plane 1 against the compare-and-select form")
        same_words(h2, o2, "plane 2 against the compare-and-select form")
        kept = int((h2 & 0x7fff != 0).sum())
        assert 0 < kept < h2.size, "the remainders must fall on both sides of the threshold (%d of %d kept)" % (kept, h2.size)


def test_specials():
    """+-0, +-inf, NaN, the largest finite f16, the first value that rounds to inf, f32 subnormals, and the threshold's neighbours."""
    F = XH_FLUSH
    pos = np.array([0.0, np.inf, np.nan, 65504.0, 65519.996, 65520.0, 65536.0, 1e-45, 1e-40, 1.1754942e-38, 2.0 ** -126, 2.0 ** -25, 2.0 ** -24,
                    np.nextafter(F, np.float32(0)), F, np.nextafter(F, np.float32(1)), 2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(1)),
                    2.0 ** -14 + 2.0 ** -25, 4094.0, 4095.99], dtype=np.float32)
    assert rne16(pos[5:6])[0] == 0x7c00 and rne16(pos[4:5])[0] == 0x7bff          # 65520 is the first f32 that rounds to inf
    r1, r2 = split_ref(pos)
    for signed1 in (False, True):
        h1, h2 = split_new(pos, signed1)
        same_words(h1, r1, "plane 1 of the non-negative specials (signed %s)" % signed1)
        same_words(h2, r2, "plane 2 of the non-negative specials (signed %s)" % signed1)
    o1, o2 = split_old(pos)
    same_words(h1, o1, "plane 1 against the compare-and-select form")
    same_words(h2, o2, "plane 2 against the compare-and-select form")
    n1, n2 = split_new(-pos, True)
    m1, m2 = split_ref(-pos)
    same_words(n1, m1, "plane 1 of the negative specials")
    same_words(n2, m2, "plane 2 of the negative specials")
    # the tie at the threshold: XH_FLUSH itself rounds UP to 2^-14 and stays; its remainder -2^-25 is flushed to +0
    h1, h2 = split_new(np.array([F], dtype=np.float32), False)
    assert h1[0] == 0x0400 and h2[0] == 0x0000
