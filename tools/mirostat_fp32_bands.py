"""How far the fp32 arithmetic of the Mirostat stage of sample_row_warp (mmtg_amd/csrc/decode.hip) lies from float64, for the two bands
of tests/test_mirostat_gpu.py: a float32 numpy evaluation in the kernel's order of operations against constraints.mirostat_filter /
mirostat_update's float64.

    python tools/mirostat_fp32_bands.py [--seeds 30] [--big-seeds 3]

No GPU.  Per row: e = exp(x - max); the survivor mass m as the kernel takes it (256 strided sequential partial sums, the 64-lane
butterfly, four waves left to right); the cut exp2(-mu) * m, against which e is compared; the kept set's mass Z as the CDF pass takes it
(256 sequential sums over contiguous chunks, then the 8-round inclusive scan); s = (log Z - (x - max)) / ln 2 of every kept id; and the
update mu - eta * (s - tau).  Reported, over random rows at three scales, V = 257, 500, 13317 and mu from 0.5 to 16 bits:
  cut       the largest | (log2 e32 - log2 cut32) - (log2 p + mu) | over the ids with p >= 2^-40: how far, in bits, the fp32 comparison
            e >= cut sits from the float64 comparison -log2 p <= mu;
  surprise  the largest | s32 - s | over the kept ids, in bits;
  update    the largest | mu'32 - mu' | / eta at eta = 0.1, tau = 2 (s's error plus the rounding of the stored mu), in bits.
The s-band is 10 x max(surprise, update), the cut band 10 x cut, both rounded up to one digit.  One JSON line."""
import argparse
import json
import math

import numpy as np

from warp_fp32_bands import block_sum

f = np.float32
LOG2E = f(1.44269504088896341)


def scan_total(e32, kept):
    """Z as the CDF pass computes it: thread t sums its contiguous chunk of the kept ids in order, then the inclusive scan
    (for o = 1, 2, .. 128: h[t] += h[t - o]); Z = h[255]."""
    V = e32.size
    chunk = (V + 255) // 256
    h = np.zeros(256, dtype=f)
    for t in range(256):
        acc = f(0)
        for v in range(t * chunk, min(V, (t + 1) * chunk)):
            if kept[v]:
                acc = f(acc + e32[v])
        h[t] = acc
    o = 1
    while o < 256:
        add = np.zeros(256, dtype=f)
        add[o:] = h[:-o]
        h = (h + add).astype(f)
        o <<= 1
    return h[255]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=30)
    ap.add_argument("--big-seeds", type=int, default=3)
    a = ap.parse_args()
    eta, tau = 0.1, 2.0
    worst = dict(cut=0.0, surprise=0.0, update=0.0)
    for V in (257, 500, 13317):
        for seed in range(a.seeds if V < 10000 else a.big_seeds):
            rng = np.random.default_rng(seed)
            for scale in (1.0, 3.0, 6.0):
                x32 = (rng.normal(size=V) * scale).astype(f)
                x = x32.astype(np.float64)
                d64 = x - x.max()
                log2p = (d64 - np.log(np.exp(d64).sum())) / math.log(2.0)
                d = (x32 - x32.max()).astype(f)
                e32 = np.exp(d).astype(f)
                m32 = block_sum(e32)
                for mu in ((0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0) if V < 10000 else (2.0, 4.0, 8.0)):
                    mu32 = f(mu + rng.uniform(-0.25, 0.25))                 # (a state the device could hold: an fp32 number)
                    mu64 = float(mu32)
                    cut32 = f(f(np.exp2(-mu32)) * m32)
                    seen = log2p >= -40.0
                    dev = np.log2(e32[seen].astype(np.float64)) - math.log2(float(cut32))
                    worst["cut"] = max(worst["cut"], float(np.abs(dev - (log2p[seen] + mu64)).max()))
                    kept = (e32 >= cut32) | (d == 0)
                    kept64 = (-log2p <= mu64) | (d64 == 0)
                    if not np.array_equal(kept, kept64):                    # an id inside the cut band: the sets may differ there
                        continue
                    Z32 = scan_total(e32, kept)
                    Z = np.exp(d64[kept]).sum()
                    s32 = ((f(np.log(Z32)) - d[kept]).astype(f) * LOG2E).astype(f)
                    s = (math.log(Z) - d64[kept]) / math.log(2.0)
                    worst["surprise"] = max(worst["surprise"], float(np.abs(s32.astype(np.float64) - s).max()))
                    up32 = (mu32 - (f(eta) * (s32 - f(tau)).astype(f)).astype(f)).astype(f)
                    up = mu64 - eta * (s - tau)
                    worst["update"] = max(worst["update"], float(np.abs(up32.astype(np.float64) - up).max()) / eta)

    def band(v):
        e = math.floor(math.log10(10.0 * v))
        return math.ceil(10.0 * v / 10.0 ** e) * 10.0 ** e

    print(json.dumps(dict(worst_fp32_error=worst, bands=dict(s=band(max(worst["surprise"], worst["update"])), cut=band(worst["cut"])))))


if __name__ == "__main__":
    main()
