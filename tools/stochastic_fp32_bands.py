"""How far the fp32 arithmetic of gumbel_candidates_kernel (mmtg_amd/csrc/decode.hip) lies from float64, for the three bands of
tests/test_stochastic_gpu.py: a float32 numpy evaluation in the kernel's order of operations against constraints.gumbel_candidates'
float64.

    python tools/stochastic_fp32_bands.py [--seeds 30] [--big-seeds 3]

No GPU.  Per row of processed logits x (fp32 numbers; a tenth of the ids banned), a score in [-40, 0] and a perturbed value in [-5, 0]
-- the ranges the test draws from; the error of cand_g grows with |score|, whose sum with t is rounded to fp32:
  mx = max x; sum of exp(x - mx) as the kernel takes it (256 strided sequential partial sums, the 64-lane butterfly, four waves left to
  right); lp = (x - mx) - log(sum); u from the hash, exactly; t = lp + -log(-log(u)); Zt = max t; for the 16 largest t:
  G = score + t; w = (gum - G) + log1mexp(t - Zt); cand_g = gum - max(0, w) - log1p(exp(-|w|)).
Reported, over random rows at three scales and V = 103, 1000, 13317:
  t       the largest | t32 - t | over the allowed ids: what can reorder two ids whose float64 t lie closer than twice that;
  lp      the largest | lp32 - lp | over the allowed ids (cand_val);
  cand_g  the largest | cand_g32 - cand_g | over the 16 ids the fp32 evaluation offers (float64 evaluated at the same ids).
A band is 10 x its value, rounded up to one digit: the device's logf / expf are not numpy's.  One JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mmtg_amd.constraints import gumbel_uniforms  # noqa: E402
from warp_fp32_bands import block_sum  # noqa: E402

f = np.float32
LN2 = f(0.69314718)


def log1mexp32(a):
    with np.errstate(divide="ignore"):
        hi = np.log((-np.expm1(a)).astype(f)).astype(f)
        lo = np.log1p((-np.exp(a).astype(f)).astype(f)).astype(f)
    return np.where(a > -LN2, hi, lo).astype(f)


def log1mexp64(a):
    with np.errstate(divide="ignore"):
        return np.where(a > -math.log(2.0), np.log(-np.expm1(a)), np.log1p(-np.exp(a)))


def row_fp32(x32, ok, u32, sb, gb, nb):
    """(t32 [V], lp32 [V], ids [nb], cand_g32 [nb]) of one row as the kernel computes them."""
    mx = x32[ok].max()
    d = (x32 - mx).astype(f)
    e = np.where(ok, np.exp(d).astype(f), f(0))
    lsum = f(np.log(block_sum(e)))
    lp = (d - lsum).astype(f)
    n32 = (-np.log((-np.log(u32)).astype(f))).astype(f)
    t = np.where(ok, (lp + n32).astype(f), f(-np.inf)).astype(f)
    zt = t.max()
    ids = np.lexsort((np.arange(t.size), -t))[:nb]
    G = (sb + t[ids]).astype(f)
    w = ((gb - G).astype(f) + log1mexp32((t[ids] - zt).astype(f))).astype(f)
    g = ((gb - np.maximum(f(0), w)).astype(f) - np.log1p(np.exp(-np.abs(w)).astype(f)).astype(f)).astype(f)
    return t, lp, ids, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=30)
    ap.add_argument("--big-seeds", type=int, default=3)
    a = ap.parse_args()
    nb = 16
    worst = dict(t=0.0, lp=0.0, cand_g=0.0)
    for V in (103, 1000, 13317):
        for seed in range(a.seeds if V < 10000 else a.big_seeds):
            rng = np.random.default_rng(seed)
            for scale in (1.0, 2.0, 6.0):
                x32 = (rng.normal(size=V) * scale).astype(f)
                ok = rng.random(V) >= 0.1
                ok[[1, 2, 100, 102]] = False
                sb, gb = f(-rng.random() * 40.0), f(-rng.random() * 5.0)
                u32 = gumbel_uniforms(np.array([seed * 7919 + V], np.uint32), 40 + seed, V)[0]
                t32, lp32, ids, g32 = row_fp32(x32, ok, u32, sb, gb, nb)
                x = x32.astype(np.float64)
                d64 = x - x[ok].max()
                lp = d64 - math.log(np.exp(d64[ok]).sum())
                t = lp + -np.log(-np.log(u32.astype(np.float64)))
                zt = t[ok].max()
                w = (float(gb) - (float(sb) + t[ids])) + log1mexp64(t[ids] - zt)
                g = float(gb) - np.maximum(0.0, w) - np.log1p(np.exp(-np.abs(w)))
                worst["t"] = max(worst["t"], float(np.abs(t32[ok].astype(np.float64) - t[ok]).max()))
                worst["lp"] = max(worst["lp"], float(np.abs(lp32[ok].astype(np.float64) - lp[ok]).max()))
                fin = np.isfinite(g)
                worst["cand_g"] = max(worst["cand_g"], float(np.abs(g32[fin].astype(np.float64) - g[fin]).max()))

    def band(v):
        e = math.floor(math.log10(10.0 * v))
        return float("%.1g" % (math.ceil(10.0 * v / 10.0 ** e) * 10.0 ** e))

    print(json.dumps(dict(worst_fp32_error=worst, bands={k: band(v) for k, v in worst.items()})))


if __name__ == "__main__":
    main()
