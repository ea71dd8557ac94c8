"""How far the fp32 arithmetic of sample_row_warp (mmtg_amd/csrc/decode.hip) lies from float64, for the bands of
tests/test_warp_gpu.py: a float32 numpy evaluation in the kernel's order of operations against constraints.warp_filter's float64.

    python tools/warp_fp32_bands.py [--seeds 30] [--big-seeds 3]

No GPU.  Per row: e = exp(x - max) and the sums of e and e (x - max) as the kernel takes them (256 strided sequential partial sums, the
64-lane butterfly, four waves left to right), log of the mass, the entropy, the typical key |(lt - (x - max)) - H|, the radix select
by accumulated mass (four passes of 256 bins; the atomics land in random order; thread 0 walks the bins), eta.  Reported: the largest
error of a key, of the accumulated mass at the cut, of a probability and of eta (both relative), over random rows at three scales and
V = 257, 500, 13317.  One JSON line."""
import argparse
import json
import math

import numpy as np

f = np.float32


def block_sum(a):
    V = a.size
    pad = np.zeros(((V + 255) // 256) * 256, dtype=f)
    pad[:V] = a
    part = np.zeros(256, dtype=f)
    for r in pad.reshape(-1, 256):
        part = (part + r).astype(f)
    w = part.reshape(4, 64)
    while w.shape[1] > 1:
        w = (w[:, :w.shape[1] // 2] + w[:, w.shape[1] // 2:]).astype(f)
    w = w[:, 0]
    return f(f(f(w[0] + w[1]) + w[2]) + w[3])


def fkey(k32):
    return k32.view(np.uint32) | np.uint32(0x80000000)          # keys are >= 0


def radix_mass(key32, e32, P, rng):
    """The kernel's select: (integer image of the cut key or None, the mass it had accumulated at the cut, inclusive)."""
    k = fkey(key32)
    prefix, mask, acc, last = np.uint32(0), np.uint32(0), f(0), f(0)
    for shift in (24, 16, 8, 0):
        idx = rng.permutation(np.flatnonzero((k & mask) == prefix))
        bins = np.zeros(256, dtype=f)
        for i, b in zip(idx, ((k[idx] >> np.uint32(shift)) & np.uint32(255)).astype(int)):
            bins[b] = f(bins[b] + e32[i])
        b = 0
        while b < 256 and not f(acc + bins[b]) >= P:
            acc = f(acc + bins[b])
            b += 1
        if b == 256:
            if shift == 24:
                return None, acc
            b = 255
        prefix, mask, last = prefix | np.uint32(b << shift), mask | np.uint32(255 << shift), bins[b]
    return prefix, f(acc + last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=30)
    ap.add_argument("--big-seeds", type=int, default=3)
    a = ap.parse_args()
    worst = dict(key=0.0, mass=0.0, probability=0.0, eta=0.0)
    for V in (257, 500, 13317):
        for seed in range(a.seeds if V < 10000 else a.big_seeds):
            rng = np.random.default_rng(seed)
            for scale in (1.0, 3.0, 6.0):
                x32 = (rng.normal(size=V) * scale).astype(f)
                x = x32.astype(np.float64)
                e = np.exp(x - x.max())
                p = e / e.sum()
                logp = (x - x.max()) - np.log(e.sum())
                H = -(p * logp).sum()
                key = np.abs(-logp - H)
                d = (x32 - x32.max()).astype(f)
                e32 = np.exp(d).astype(f)
                m32, s32 = block_sum(e32), block_sum((e32 * d).astype(f))
                lt = f(np.log(m32))
                H32 = f(lt - f(s32 / m32))
                key32 = np.abs(((lt - d).astype(f) - H32).astype(f))
                worst["key"] = max(worst["key"], float(np.abs(key32.astype(np.float64) - key).max()))
                worst["probability"] = max(worst["probability"], float(np.abs((e32.astype(np.float64) / float(m32)) / p - 1).max()))
                for tp in ((0.2, 0.5, 0.9, 0.95) if V < 10000 else (0.5, 0.9)):
                    cut, mass32 = radix_mass(key32, e32, f(f(tp) * m32), rng)
                    if cut is not None:
                        worst["mass"] = max(worst["mass"], abs(float(mass32) / float(m32) - float(p[fkey(key32) <= cut].sum())))
                for ec in (3e-4, 2e-3, 0.05):
                    eta = min(ec, math.sqrt(ec) * math.exp(-H))
                    eta32 = min(f(ec), f(np.sqrt(f(ec))) * f(np.exp(-H32)))
                    worst["eta"] = max(worst["eta"], abs(float(eta32) / eta - 1))
    print(json.dumps(dict(worst_fp32_error=worst, bands=dict(key=1e-4, mass=2e-5, probability=1e-4))))


if __name__ == "__main__":
    main()
