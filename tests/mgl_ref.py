"""The per-modality guided validation loss: the float64 reference of mmtg_guided_loss_multi (the rule in include/mmtg_hip.h), the error
bounds of its fp32 evaluation, a float32 restatement of the kernel's expressions (csrc/guidance_train.hip: guided_multi_row_kernel,
guided_sample_kernel) and the cases of tests/test_mgloss_ops_gpu.py (tests/test_mgloss_cpu.py walks the same list).

Convention (as tests/cfg_ref.py): torch on the CPU; the K logits matrices come in their storage type and are widened exactly; the K
lse vectors are the fp32 values the kernel is given; a scale is the fp32 value the kernel receives and w_k = fl32(s_k - 1) is formed
in fp32 FIRST, as the entry forms it on the host, so the reference uses the very weights the kernel uses.

The bounds, by counting rounded fp32 operations exactly as cfg_ref does (EPS = 2^-24, TR = 2^-21 per exponential stage and for logf):

  lc = x_0 - lse_0, l_k = x_k - lse_k      one rounding each: dlc = EPS |lc|, dl_k = EPS |l_k|
  d_k = lc - l_k                            dd_k = dlc + dl_k + EPS |d_k|
  g_0 = lc;  g_k = g_{k-1} + w_k d_k        dg_k = dg_{k-1} + |w_k| dd_k + EPS |w_k d_k| + EPS |g_k|     (dg_0 = dlc; the product, the sum;
                                            a fused multiply-add rounds once, so this counts one rounding too many, never too few)
  L(g), nll, sample_ce, ce                  cfg_ref's lines, with the stage and depth counts of the path the ROW takes:
      all K row pointers 16-byte aligned    slices of 2048 logits, eight per thread, and a tail element: NST = ceil(V / 2048) + 11 stages
                                            (one running-max move per slice, one for the tail, six butterfly stages, three wave merges,
                                            the element's own exponential), DEPTH = 8 ceil(V / 2048) + 10 additions
      otherwise                             one logit per thread and trip, T = ceil(V / 256) trips: NST = T + 10, DEPTH = T + 9
  An fp32 matrix whose row stride is no multiple of 16 bytes mixes the two paths row by row (ODD: rows 0, 4, 8, ... are aligned), so
  the counts are per row.  Nothing here is fitted to what the kernel gives."""
import functools
import math

import numpy as np
import torch

from cfg_ref import EPS, F64, TR, loss_rows, row_labels

MAX_BRANCHES, MAX_TUPLES = 4, 8


def weights(tuples):
    """float64 [G, K - 1]: fl32(fl32(s) - 1), the weights the entry hands to the kernel"""
    return (np.asarray(tuples, dtype=np.float32) - np.float32(1.0)).astype(np.float64).reshape(len(tuples), -1)


def vector_rows(M, ldl, bf, offs):
    """bool [M]: the rows whose K pointers are all 16-byte aligned (offs: each matrix's base offset in bytes from an aligned address)"""
    es = 2 if bf else 4
    m = torch.arange(M)
    ok = torch.ones(M, dtype=torch.bool)
    for o in offs:
        ok &= (o + m * ldl * es) % 16 == 0
    return ok


def trip_counts(V, vec):
    """(NST, DEPTH) per row, float64 [M]"""
    c, t = math.ceil(V / 2048), math.ceil(V / 256)
    nst = torch.where(vec, torch.tensor(float(c + 11)), torch.tensor(float(t + 10))).to(F64)
    depth = torch.where(vec, torch.tensor(float(8 * c + 10)), torch.tensor(float(t + 9))).to(F64)
    return nst, depth


def reference(mats, lses, targets, P, V, tuples, batch_den, offs=None):
    """mats: K logits matrices [M, ldl] in their storage type (mats[0] the conditional one); lses: K fp32 [M]; tuples: G tuples of
    K - 1 scales.  Returns float64 tensors: nll [G, M] (0 outside the loss rows), sample_ce [G, B], ce [G], allow_nll, allow_sample,
    allow_ce and dg_max [G, M], the row's largest dg."""
    K = len(mats)
    B, L = targets.shape
    Tt = P + L
    ntok = Tt - 1 - P
    M = B * Tt
    rows = loss_rows(B, P, L)
    lab = row_labels(targets, P, V)
    bf = mats[0].dtype == torch.bfloat16
    vec = vector_rows(M, mats[0].shape[1], bf, [0] * K if offs is None else offs)
    nst, depth = trip_counts(V, vec)
    ls = [x[:, :V].to(F64) - l.to(F64)[:, None] for x, l in zip(mats, lses)]
    lc, dlc = ls[0], EPS * ls[0].abs()
    ds = [lc - lk for lk in ls[1:]]
    dds = [dlc + EPS * lk.abs() + EPS * d.abs() for lk, d in zip(ls[1:], ds)]
    den = float(np.float32(batch_den))
    out = {k: [] for k in ("nll", "allow_nll", "sample_ce", "allow_sample", "ce", "allow_ce", "dg_max")}
    for w in weights(tuples):
        g, dg = lc, dlc
        for wk, d, dd in zip(w, ds, dds):
            wk = float(wk)
            g = g + wk * d
            dg = dg + abs(wk) * dd + EPS * (wk * d).abs() + EPS * g.abs()
        mx = g.max(1).values
        a = g - mx[:, None]
        e = a.exp()
        S = e.sum(1)
        p = e / S[:, None]
        relS = (p * (nst[:, None] * TR + 3 * EPS * a.abs())).sum(1) + depth * EPS
        Lg = mx + S.log()
        dL = dg.max(1).values - torch.log1p(-relS) + TR * S.log().abs() + EPS * Lg.abs()
        nll = Lg - g.gather(1, lab[:, None])[:, 0]
        dnll = dL + dg.gather(1, lab[:, None])[:, 0] + EPS * nll.abs() + 1e-300
        nll = torch.where(rows, nll, torch.zeros_like(nll))
        dnll = torch.where(rows, dnll, torch.zeros_like(dnll))          # a row outside the loss rows is exactly 0
        per, dper = nll.view(B, Tt)[:, P:Tt - 1], dnll.view(B, Tt)[:, P:Tt - 1]
        smp = per.sum(1) / ntok
        dsmp = (dper.sum(1) + (ntok - 1) * EPS * per.abs().sum(1)) / ntok + EPS * smp.abs() + 1e-300
        ce = smp.sum() / den
        dce = dsmp.sum() / den + (B + 1) * EPS * smp.abs().sum() / den + 1e-300
        for k, v in zip(out, (nll, dnll, smp, dsmp, ce, dce, dg.max(1).values)):
            out[k].append(v)
    return {k: torch.stack(v) for k, v in out.items()}


def reference32(mats, lses, targets, P, V, tuples, batch_den):
    """The kernel's expressions in float32 (torch on the CPU, its own summation order): nll [G, M], sample_ce [G, B], ce [G]"""
    f = torch.float32
    B, L = targets.shape
    Tt = P + L
    rows = loss_rows(B, P, L)
    lab = row_labels(targets, P, V)
    ls = [x[:, :V].to(f) - l[:, None] for x, l in zip(mats, lses)]
    nlls, smps, ces = [], [], []
    for t in tuples:
        g = ls[0]
        for s, lk in zip(t, ls[1:]):
            w = torch.tensor(s, dtype=f) - torch.tensor(1.0, dtype=f)
            g = g + w * (ls[0] - lk)
        mx = g.max(1).values
        Lg = mx + torch.log(torch.exp2((g - mx[:, None]) * np.float32(1.4426950408889634)).sum(1))
        nll = torch.where(rows, Lg - g.gather(1, lab[:, None])[:, 0], torch.zeros((), dtype=f))
        smp = nll.view(B, Tt)[:, P:Tt - 1].sum(1) / np.float32(Tt - 1 - P)
        nlls.append(nll)
        smps.append(smp)
        ces.append(smp.sum() / np.float32(batch_den))
    return torch.stack(nlls), torch.stack(smps), torch.stack(ces)


# ---------------------------------------------------------------- the cases
B = 2
PLS = [(0, 2), (3, 5)]
# the tail alone (1 .. 7), one slice of eight and its tail (8, 9), a wave's and a workgroup's edge in the tail path (255 .. 257), one
# full slice (2047 .. 2049), the two slices in flight (4095 .. 4097), the odd trailing slice behind them (6145), a second trip of the
# two-slice loop (8193), the flagship width (13317)
VS = [1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8193, 13317]
KS = [2, 3, 4]
ODD = (255, 257)            # V, ldl of the fp32 case with an odd row stride
OFF = (257, 260)            # V, ldl of the fp32 case where ONE matrix (the last) starts 4 bytes off a 16-byte boundary
ONE = [(1.5, 3.0, 0.5)]
# 0, 1 and 7.5 mixed: three zeros (weight -2 on lc), an all-ones tuple, two equal tuples (2 and 4)
MIXED = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (7.5, 1.0, 0.0), (1.0, 7.5, 1.0), (7.5, 1.0, 0.0), (0.0, 7.5, 1.0)]
EIGHT = [(1.5, 3.0, 0.5), (0.0, 1.0, 7.5), (1.0, 1.0, 1.0), (3.0, 0.0, 1.0), (1.0, 1.5, 1.0), (7.5, 7.5, 7.5), (1.0, 1.0, 1.0), (0.5, 2.0, 1.0)]


def tuple_sets(K):
    """the three tuple sets at K matrices: each tuple cut to its first K - 1 scales"""
    return [[t[:K - 1] for t in ts] for ts in (ONE, MIXED, EIGHT)]


def padded(V):
    return (V + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def _base(V, ldl, P, L, bf):
    Tt = P + L
    M = B * Tt
    gen = torch.Generator().manual_seed(200000 * int(bf) + 10 * V + L)
    xs = []
    for _ in range(MAX_BRANCHES):
        x = torch.full((M, ldl), 1e4)
        x[:, :V] = torch.randn(M, V, generator=gen) * 4.0
        xs.append(x)
    tg = torch.randint(0, V, (B, L), generator=gen)
    if L == 2:
        tg[0, 1], tg[1, 1] = -1, V + 5
    else:
        tg[0, 1], tg[0, 3], tg[1, 2] = -1, V, V + 5
        tg[1, 0] = V + 9                        # (column 0 is never a label)
    return xs, tg


@functools.lru_cache(maxsize=None)
def case(V, ldl, P, L, bf, K):
    """K logits matrices [M, ldl] in their storage type (normal times 4; a loss row of matrix 0 and one of the last negative carry a
    +60 and a -60 outlier; the columns >= V hold 1e4, which a kernel that read them would show), their fp32 row lse (the fp32
    rounding of the float64 log-sum-exp of the stored values) and targets [B, L] with the labels -1, V and V + 5 planted."""
    xs, tg = _base(V, ldl, P, L, bf)
    Tt = P + L
    dt = torch.bfloat16 if bf else torch.float32
    mats = []
    for k in range(K):
        x = xs[k].clone()
        if k == 0 or k == K - 1:
            m = (P if L > 2 else Tt + P) if k == 0 else Tt + P          # loss rows both
            x[m, 0] += 60.0
            x[m, V - 1] -= 60.0
        mats.append(x.to(dt))
    lses = [torch.logsumexp(x[:, :V].to(F64), 1).float() for x in mats]
    return tuple(mats), tuple(lses), tg


def geometries():
    """(V, ldl, P, L, bf, off) of every case; off: None, or the byte offset of the LAST matrix's base from a 16-byte boundary"""
    out = [(V, padded(V), P, L, bf, None) for bf in (False, True) for (P, L) in PLS for V in VS]
    out.append((ODD[0], ODD[1], 3, 5, False, None))
    out.append((OFF[0], OFF[1], 3, 5, False, 4))
    return out


def offsets(K, off):
    return [0] * (K - 1) + [off or 0]


def geo_id(g):
    return "V%d-ld%d-P%d-L%d-%s%s" % (g[:4] + ("bf16" if g[4] else "f32", "-off%d" % g[5] if g[5] else ""))
