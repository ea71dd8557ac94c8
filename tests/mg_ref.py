"""Per-modality guidance: the inputs of the kernel tests, the float64 reference (constraints.modality_guidance_scores) and what the
fp32 kernel may differ from it by.

The allowance, per prompt (a float64 [N]), derived by counting rounded fp32 operations as tests/cfg_ref.py does (EPS = 2^-24):

  the K row log-sum-exps.  The kernel computes each itself, within cfg_ref.lse_allow of the exact one.  An error of L(c) moves every lc
  of the row alike, and lc enters g with the weight 1 + sum_k w_k (w_k = s_k - 1); an error of L(x_k) moves every l_k alike, and l_k
  enters with -w_k:
      |1 + sum_k w_k| lse_allow(c) + sum_k |w_k| lse_allow(x_k)
  the rule's own operations, each at EPS times the magnitude it rounds, per id, the row's largest taken:
      lc = c - L(c)                 dlc = EPS |lc|
      l_k = x_k - L(x_k)            dl_k = EPS |l_k|
      d_k = lc - l_k                dd_k = dlc + dl_k + EPS |d_k|
      w_k = s_k - 1                 EPS |w_k|, so EPS |w_k d_k| in the product
      g_k = g_{k-1} + w_k d_k       dg_k = dg_{k-1} + |w_k| dd_k + 2 EPS |w_k d_k| + EPS |g_k|      (dg_0 = dlc; the product and w_k's own
                                    rounding; a fused multiply-add rounds once, so this counts one rounding too many, not too few)
  That is decode_allow's construction (cfg_ref.py) with the rule's operations written out for K - 1 branches.  Nothing in it is fitted
  to what the kernel gives."""
import functools

import numpy as np
import torch

from cfg_ref import EPS, lse_allow
from mmtg_amd.constraints import _log_softmax64, modality_guidance_scores

NINF = float("-inf")
VS = [1, 2, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 4097, 13317]
# the scale sets per K (every value from {0, 0.5, 1, 1.5, 3, 7.5}); the second of each K puts a negative weight on lc
SCALE_SETS = {2: [(3.0,), (0.0,), (7.5,), (1.0,)],
              3: [(3.0, 1.5), (0.0, 0.5), (7.5, 0.0), (1.0, 1.0)],
              4: [(3.0, 1.5, 0.5), (0.0, 0.0, 0.0), (7.5, 1.0, 3.0), (1.0, 1.0, 1.0)]}


def aligned_ld(V):
    return (V // 8 + 1) * 8         # a multiple of 8 above V: 16-byte aligned rows, at least one column of padding


def odd_ld(V):
    return V + 1 if V % 2 == 0 else V + 2


@functools.lru_cache(maxsize=None)
def case(V, K, N):
    """float32 [K, N, V]: normal times 4; prompt min(1, N - 1) carries a +60 and a -60 outlier in its own row (as cfg_ref.case).
    Planted: with V >= 2 id V // 2 of prompt 0 is -inf in branch 1 only; with N >= 3 the last prompt's row of the last branch is
    all -inf."""
    gen = torch.Generator().manual_seed(7919 * V + 31 * K + N)
    x = (torch.randn(K, N, V, generator=gen) * 4.0).numpy().astype(np.float32)
    b = min(1, N - 1)
    x[0, b, 0] += 60.0
    x[0, b, V - 1] -= 60.0
    if V >= 2:
        x[1, 0, V // 2] = NINF
    if N >= 3:
        x[K - 1, N - 1, :] = NINF
    x.setflags(write=False)
    return x


def padded(x, ld, fill=1e4):
    """[K, N, V] as the kernel takes it: float32 [K N, ld], branch k of prompt b in row k N + b, columns >= V holding `fill`"""
    K, N, V = x.shape
    out = np.full((K * N, ld), fill, np.float32)
    out[:, :V] = x.reshape(K * N, V)
    return out


def multi_allow(x, scales):
    """What mmtg_decode_guidance_multi's out may differ from modality_guidance_scores(x, scales) by, per prompt: float64 [N] (0 for a
    prompt one of whose rows has no distribution: its ids are all -inf, exactly).  x: float32 [K, N, V]."""
    K, N, V = x.shape
    w = [float(np.float32(s)) - 1.0 for s in scales]
    dead = np.array([[not np.isfinite(x[k, b]).any() for b in range(N)] for k in range(K)]).any(0)
    live = np.where(~dead)[0]
    out = np.zeros(N)
    if live.size == 0:
        return out
    xl = x[:, live].astype(np.float64)
    t = [torch.from_numpy(xl[k]) for k in range(K)]
    la = [lse_allow(tk, V).numpy() for tk in t]
    lse_part = abs(1.0 + sum(w)) * la[0] + sum(abs(wk) * lak for wk, lak in zip(w, la[1:]))
    ls = [_log_softmax64(xl[k]) for k in range(K)]
    fin = np.ones(ls[0].shape, bool)
    for l in ls:
        fin &= np.isfinite(l)
    with np.errstate(invalid="ignore"):
        dlc = EPS * np.abs(ls[0])
        g, dg = ls[0].copy(), dlc.copy()
        for wk, lk in zip(w, ls[1:]):
            d = ls[0] - lk
            dd = dlc + EPS * np.abs(lk) + EPS * np.abs(d)
            g = g + wk * d
            dg = dg + abs(wk) * dd + 2 * EPS * np.abs(wk * d) + EPS * np.abs(g)
    ops_part = np.where(fin, dg, 0.0).max(1)
    out[live] = lse_part + ops_part
    return out


@functools.lru_cache(maxsize=None)
def reference(V, K, N, scales):
    """(want float64 [N, V], allow float64 [N]) of case(V, K, N) under `scales`"""
    x = case(V, K, N)
    want = modality_guidance_scores(x, scales)
    allow = multi_allow(x, scales)
    want.setflags(write=False)
    allow.setflags(write=False)
    return want, allow
