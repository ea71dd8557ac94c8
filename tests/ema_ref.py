"""What the weight-averaging tests share: the float64 formula of one update, its float32 restatement and the error bound.

One update is ema <- fmaf(w, p - ema, ema) in fp32: the difference is rounded once (at most 2^-24 |p - e| relative to the exact
difference, scaled by w on its way into the result) and the fused multiply-add is rounded once (half a spacing of the result).
Against the float64 value of w (p - e) + e the result is therefore within

    0.5 * spacing32(max(|ref|, |got|)) + 2^-24 * w * |p - e|

and where p == e it is e bit for bit.  The bound follows from the two roundings; it is not fitted to any kernel's output."""
import numpy as np


def w32(w):
    """w as the kernel receives it: rounded once to fp32"""
    return float(np.float32(w))


def ema_ref64(e, p, w):
    """float64 value of w (p - e) + e for fp32 arrays e, p and the fp32 weight w"""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return w32(w) * (p - e) + e


def ema_restated32(e, p, w):
    """the update in numpy: the difference rounded to fp32, product and sum formed in float64 (the product of two fp32 values is exact
    there), rounded once to fp32; a result that equals e is e (the kernel's select: it keeps the sign of an e of -0)"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d = (p - e).astype(np.float32)
    r = (w32(w) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)
    return np.where(r == e, e, r)


def ema_bound(e, p, w, got):
    """elementwise bound on |got - ema_ref64(e, p, w)|"""
    ref = ema_ref64(e, p, w)
    big = np.maximum(np.abs(ref), np.abs(np.asarray(got, dtype=np.float64))).astype(np.float32)
    diff = np.abs(np.asarray(p, dtype=np.float64) - np.asarray(e, dtype=np.float64))
    return 0.5 * np.spacing(big).astype(np.float64) + 2.0 ** -24 * w32(w) * diff


def check_update(e, p, w, got, what=""):
    """got (fp32) against the float64 formula on the fp32 state e it started from; prints the worst ratio to the bound; -> it"""
    e, p, got = (np.asarray(x, dtype=np.float32) for x in (e, p, got))
    err = np.abs(got.astype(np.float64) - ema_ref64(e, p, w))
    bound = ema_bound(e, p, w, got)
    ratio = float((err / bound).max())
    print("%s: max |got - ref| / bound = %.7f over %d elements" % (what, ratio, e.size))
    assert np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, ratio)
    same = p == e
    assert (got.view(np.int32)[same] == e.view(np.int32)[same]).all(), what      # p == e: e bit for bit
    return ratio
