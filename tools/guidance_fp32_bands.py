"""How far the fp32 arithmetic of decode_guidance_kernel (mmtg_amd/csrc/decode_guidance.hip) lies from float64, for the band of
tests/test_guidance_gpu.py: a float32 numpy evaluation in the kernel's order of operations against constraints.guidance_scores.

    python tools/guidance_fp32_bands.py [--seeds 3]

No GPU.  Per row, as the kernel takes it: every one of 256 threads folds its share into a running (max, sum of exp(x - max)) pair -- a
16-byte aligned row in passes of 8 float4 per thread (the pass's 32 logits: their maximum, the sum of exp(x - max) in load order, then
one merge into the pair), the tail and an unaligned row one logit at a time (one merge each); the 64-lane butterfly (xor 32 .. 1); the
four waves left to right; L = max + log(sum).  Then lc = c - L(c), lu = u - L(u), g = lu + s * (lc - lu).  (The device may contract a
product and a sum into one fused operation, and its expf / logf are not numpy's: the test's band is twice what is found here.)

The band's form is k * 2^-24 * (1 + 2 s) * M with M = max(|c|inf + |L(c)|, |u|inf + |L(u)|): each of lc and lu carries the rounding of a
difference of numbers up to M, g that of three more operations on them, two of which are scaled by s.  Reported: the worst k over
V = 257, 500, 13317, three value scales, both load paths, s in {0, 1, 1.5, 3, 7.5} and the seeds; the test's k is twice that, rounded up
to an integer.  One JSON line."""
import argparse
import json
import math

import numpy as np

f = np.float32
SCALES = (0.0, 1.0, 1.5, 3.0, 7.5)
NINF = f(-np.inf)


def lse_merge(m, s, om, os_):
    """(max, sum) pairs merged element-wise, as the kernel's lse_merge: a pair whose max is -inf holds nothing."""
    nm = np.maximum(m, om)
    with np.errstate(invalid="ignore"):
        out = (s * np.exp((m - nm).astype(f)).astype(f)).astype(f) + (os_ * np.exp((om - nm).astype(f)).astype(f)).astype(f)
    return nm, np.where(nm == NINF, f(0), out.astype(f)).astype(f)


def row_lse(x, aligned=True):
    """L(x) = max + log(sum exp(x - max)) of a float32 row in the kernel's order; -inf for a row without a finite entry."""
    x = np.asarray(x, dtype=f)
    V = x.size
    m, s = np.full(256, NINF, dtype=f), np.zeros(256, dtype=f)
    done = 0
    if aligned:
        nvec = V >> 2
        x4 = np.full((((nvec + 2047) // 2048) * 2048, 4), NINF, dtype=f)
        x4[:nvec] = x[:nvec * 4].reshape(nvec, 4)
        for base in range(0, nvec, 2048):
            r = x4[base:base + 2048].reshape(8, 256, 4).transpose(1, 0, 2).reshape(256, 32)        # [thread, its 32 logits in load order]
            pm = r.max(axis=1)
            ps = np.zeros(256, dtype=f)
            with np.errstate(invalid="ignore"):
                for e in range(32):
                    ps = (ps + np.exp((r[:, e] - pm).astype(f)).astype(f)).astype(f)
            live = pm != NINF
            nm, ns = lse_merge(m, s, np.where(live, pm, NINF), np.where(live, ps, f(0)))
            m, s = np.where(live, nm, m), np.where(live, ns, s)
        done = nvec << 2
    tail = x[done:]
    pad = np.full(((tail.size + 255) // 256) * 256, NINF, dtype=f)
    pad[:tail.size] = tail
    for r in pad.reshape(-1, 256):
        live = r != NINF
        nm, ns = lse_merge(m, s, r, np.ones(256, dtype=f))
        m, s = np.where(live, nm, m), np.where(live, ns, s)
    m, s = m.reshape(4, 64), s.reshape(4, 64)
    o = 32
    while o:
        idx = np.arange(64) ^ o
        m, s = lse_merge(m, s, m[:, idx], s[:, idx])
        o >>= 1
    mm, ss = m[0, 0:1], s[0, 0:1]
    for w in range(1, 4):
        mm, ss = lse_merge(mm, ss, m[w, 0:1], s[w, 0:1])
    return NINF if mm[0] == NINF else f(mm[0] + f(np.log(ss[0])))


def kernel_f32(c, u, scale, aligned=True, V=None):
    """The kernel's result for one pair of float32 rows, cut at V (default: all of them)."""
    c, u = np.asarray(c, dtype=f), np.asarray(u, dtype=f)
    V = c.size if V is None else V
    c, u = c[:V], u[:V]
    Lc, Lu = row_lse(c, aligned), row_lse(u, aligned)
    with np.errstate(invalid="ignore"):
        lc, lu = (c - Lc).astype(f), (u - Lu).astype(f)
        g = (lu + (f(scale) * (lc - lu).astype(f)).astype(f)).astype(f)
    return np.where((c == NINF) | (u == NINF), NINF, g).astype(f)


def lse64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return -np.inf if m == -np.inf else m + math.log(np.exp(x - m).sum())


def band_unit(c, u, scale):
    """2^-24 * (1 + 2 s) * M of one pair (float64): what k multiplies."""
    c, u = np.asarray(c, dtype=np.float64), np.asarray(u, dtype=np.float64)
    fin = lambda x: np.abs(x[np.isfinite(x)]).max() if np.isfinite(x).any() else 0.0
    M = max(fin(c) + abs(lse64(c)), fin(u) + abs(lse64(u)))
    return 2.0 ** -24 * (1.0 + 2.0 * scale) * M


def main():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from mmtg_amd.constraints import guidance_scores
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    worst, where = 0.0, None
    for V in (257, 500, 13317):
        for seed in range(a.seeds):
            rng = np.random.default_rng(seed)
            for sc in (1.0, 3.0, 6.0):
                c = (rng.normal(size=V) * sc).astype(f)
                u = (rng.normal(size=V) * sc).astype(f)
                for aligned in (True, False):
                    for s in SCALES:
                        got = kernel_f32(c, u, s, aligned).astype(np.float64)
                        k = float(np.abs(got - guidance_scores(c, u, s)).max() / band_unit(c, u, s))
                        if k > worst:
                            worst, where = k, dict(V=V, seed=seed, value_scale=sc, aligned=aligned, s=s)
    print(json.dumps(dict(worst_k=worst, at=where, test_k=int(math.ceil(2.0 * worst)))))


if __name__ == "__main__":
    main()
