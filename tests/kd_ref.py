"""Distillation of a teacher's (guided) distribution: the float64 reference of mmtg_distill_fwd, mmtg_loss_bwd_kd and
mmtg_loss_bwd_kd_x3 (the rule in include/mmtg_hip.h) and the error bounds of their fp32 evaluation (csrc/distill.hip).

Convention (as tests/cfg_ref.py): torch on the CPU; logits come in their storage type and are widened exactly; every lse vector and
coef are the fp32 values the kernel is given; scale, gscale, lm_coef and the coefficient w are the fp32 values it receives.  The row
factor cf = (coef[b] * gscale) + lm_coef is formed in float32 in the kernel's order, so the reference uses the kernel's cf exactly.

The bounds, derived by counting rounded fp32 operations (EPS = 2^-24 is half an ulp relative; TR = 2^-21 covers one exponential
stage, as derived in tests/cfg_ref.py; nothing here is fitted to a kernel's output):

  forward, per element of a loss row
    g (and dg) as in cfg_ref: lc = c - lse_c, lu = u - lse_u, d = lc - lu, g = lu + s d:
        dg = dlu + s dd + EPS |s d| + EPS |g|        (no negative: g = lc, dg = EPS |lc|)
    logp = x - lse                          dlogp = EPS |logp|
    h = g - logp                            dh = dg + dlogp + EPS |h|
  the running triple.  The kernel's weight of element v is e_v = exp(g_v - running max), carried through NST = ceil(V / 2048) + 11
  rescaling stages and DEPTH = 8 ceil(V / 2048) + 10 additions exactly as cfg_ref counts them for mmtg_guided_loss (one slice of
  2048 per sweep of the workgroup, six butterfly stages, three merges).  Relative to the exact q_v, and up to the common factor
  e^(-max) that cancels in A / S, the weight is q_v (1 + a_v) with
        |a_v| <= abar_v = expm1(dg_v) + NST TR + 3 EPS |max g - g_v| + (DEPTH + 2) EPS      (+ 1 EPS: the product e h in A)
  Lg = max + log S:                         dL = max_v dg - log(1 - relS) + TR |log S| + EPS |Lg|       (cfg_ref's dL)
  A / S = sum q (1 + a) (h + dh) / sum q (1 + a'):   with E = sum q h, dN = sum q (abar |h| + (1 + abar) dh), dD = sum q abar,
        d(A / S) = (dN + |E| dD) / (1 - dD) + 5 EPS |E|        (the division: within OpenCL's 2.5 ulp)
  kd_row = A / S - Lg                       dkd_row = d(A / S) + dL + EPS |kd_row|
  kd_sample, kd: sums of ntok rows / B samples in any order, as cfg_ref's sample_ce and ce.

  backward, per element
    p = expf(x - lse)                       dp = p (EPS |logp| + TR)
    q = exp(g - Lg'), Lg' within dL of Lg   dq = q (expm1(dg + dL) + 3 EPS |g - Lg| + TR)
    t1 = cf (p - [label])                   dt1 = |cf| (dp + EPS |p - [label]|) + EPS |t1|
    t2 = w (p - q)                          dt2 = w (dp + dq + EPS |p - q|) + EPS |t2|
    d = t1 + t2                             dd = dt1 + dt2 + EPS |d|       (a fused multiply-add rounds less, never more)
  a row without the term (w = 0 or t < P): d = t1, dd = dt1.  Storage: fp32 as it is; bf16 adds half a bf16 ulp, 2^-8 (|d| + dd);
  the (hi | lo) planes are compared as hi + lo and add 2^-16 (|d| + dd) -- lo is the bf16 rounding of a remainder below half an ulp
  of hi -- and bf16's smallest subnormal, 2^-133.
"""
import functools
import math

import numpy as np
import torch

import cfg_ref as C

EPS, TR, F64 = C.EPS, C.TR, C.F64
B, PLS, ODD = C.B, C.PLS, C.ODD
# cfg_ref's set and V +- 1 where csrc/distill.hip changes path: a thread's second 8-wide slice begins at V = 2056
VS = list(C.VS) + [2047, 2048, 2049, 2055, 2056, 2057]
SCALES = [None, 0.0, 1.0, 1.5, 3.0, 7.5]         # None: no negative (null uncond)
GSCALE, LM_COEF, KD_COEF = 2.0, 0.015625, 0.375
TINY = 1e-300


def stages(V):
    return math.ceil(V / 2048) + 11, 8 * math.ceil(V / 2048) + 10


def row_factor(coef, gscale, lm_coef, B_, P, L):
    """float64 [M] of the kernel's fp32 cf: (coef[b] * gscale) + lm_coef on the loss rows, 0 + lm_coef on rows t < P, and active [M]"""
    Tt = P + L
    t = torch.arange(B_ * Tt) % Tt
    b = torch.arange(B_ * Tt) // Tt
    base = (coef.float() * torch.tensor(gscale, dtype=torch.float32))[b]
    cf = torch.where(t >= P, base, torch.zeros_like(base)) + torch.tensor(lm_coef, dtype=torch.float32)
    active = (t + 1 < Tt) & ((t >= P) | (float(np.float32(lm_coef)) != 0.0))
    return cf.to(F64), active


def all_labels(topic_ids, targets, P, V):
    """int64 [M]: cat(topic_ids, targets)[b, t + 1] clamped into [0, V) for t + 1 < Tt; 0 on each sample's last row"""
    B_, L = targets.shape
    seq = targets if P == 0 else torch.cat([topic_ids, targets], 1)
    lab = torch.zeros(B_, P + L, dtype=torch.long)
    lab[:, :-1] = seq[:, 1:].clamp(0, V - 1)
    return lab.view(-1)


def teacher_g(c, u, lse_c, lse_u, s, V):
    """g [M, V] and dg [M, V] in float64"""
    lc = c[:, :V].to(F64) - lse_c.to(F64)[:, None]
    if u is None:
        return lc, EPS * lc.abs()
    s = float(np.float32(s))
    lu = u[:, :V].to(F64) - lse_u.to(F64)[:, None]
    dlc, dlu = EPS * lc.abs(), EPS * lu.abs()
    d = lc - lu
    dd = dlc + dlu + EPS * d.abs()
    g = lu + s * d
    return g, dlu + s * dd + EPS * (s * d).abs() + EPS * g.abs()


def forward(x, lse, c, u, lse_c, lse_u, s, P, L, V, batch_den):
    """x [M, >= V] student logits in their storage type (or float64), lse its row lse (fp32, or float64 for the exact rule).
    Returns float64 tensors: kd_row, Lg [M] (0 outside the loss rows), kd_sample [B], kd, their allow_*, and g, dg, q, dL for the
    backward."""
    M = x.shape[0]
    B_ = M // (P + L)
    Tt = P + L
    ntok = Tt - 1 - P
    rows = C.loss_rows(B_, P, L)
    nst, depth = stages(V)
    den = float(np.float32(batch_den))
    g, dg = teacher_g(c, u, lse_c, lse_u, s, V)
    logp = x[:, :V].to(F64) - lse.to(F64)[:, None]
    h = g - logp
    dh = dg + EPS * logp.abs() + EPS * h.abs()
    mx = g.max(1).values
    a = g - mx[:, None]
    e = a.exp()
    S = e.sum(1)
    q = e / S[:, None]
    Lg = mx + S.log()
    relS = (q * (nst * TR + 3 * EPS * a.abs())).sum(1) + depth * EPS
    dL = dg.max(1).values - torch.log1p(-relS) + TR * S.log().abs() + EPS * Lg.abs()
    abar = torch.expm1(dg) + nst * TR + 3 * EPS * a.abs() + (depth + 3) * EPS
    E = (q * h).sum(1)
    dN = (q * (abar * h.abs() + (1 + abar) * dh)).sum(1)
    dD = (q * abar).sum(1)
    dratio = (dN + E.abs() * dD) / (1 - dD) + 5 * EPS * E.abs()
    row = (q * (g - Lg[:, None] - logp)).sum(1)
    drow = dratio + dL + EPS * row.abs() + TINY
    zero = torch.zeros_like(row)
    row, drow = torch.where(rows, row, zero), torch.where(rows, drow, zero)
    Lg_out, dLg_out = torch.where(rows, Lg, zero), torch.where(rows, dL + TINY, zero)
    per, dper = row.view(B_, Tt)[:, P:Tt - 1], drow.view(B_, Tt)[:, P:Tt - 1]
    smp = per.sum(1) / ntok
    dsmp = (dper.sum(1) + (ntok - 1) * EPS * per.abs().sum(1)) / ntok + EPS * smp.abs() + TINY
    kd = smp.sum() / den
    dkd = dsmp.sum() / den + (B_ + 1) * EPS * smp.abs().sum() / den + TINY
    return {"kd_row": row, "allow_row": drow, "kd_lg": Lg_out, "allow_lg": dLg_out, "kd_sample": smp, "allow_sample": dsmp,
            "kd": kd, "allow_kd": dkd, "g": g, "dg": dg, "q": q, "Lg": Lg, "dL": dL, "logp": logp, "rows": rows}


def backward(x, lse, fwd, topic_ids, targets, coef, gscale, lm_coef, w, P, V, Vpad):
    """d [M, Vpad] float64 and its fp32 allowance [M, Vpad]; fwd: forward()'s result on the same inputs.  Rows that are not active
    and the columns >= V are exactly 0."""
    M = x.shape[0]
    B_, L = targets.shape
    cf, active = row_factor(coef, gscale, lm_coef, B_, P, L)
    lab = all_labels(topic_ids, targets, P, V)
    w = float(np.float32(w))
    logp = x[:, :V].to(F64) - lse.to(F64)[:, None]
    p = logp.exp()
    dp = p * (EPS * logp.abs() + TR)
    one = torch.zeros(M, V, dtype=F64)
    one[torch.arange(M), lab] = 1.0
    t1 = cf[:, None] * (p - one)
    dt1 = cf.abs()[:, None] * (dp + EPS * (p - one).abs()) + EPS * t1.abs()
    kdrow = (fwd["rows"] & (w != 0.0))[:, None]
    q, g, Lg = fwd["q"], fwd["g"], fwd["Lg"]
    dq = q * (torch.expm1(fwd["dg"] + fwd["dL"][:, None]) + 3 * EPS * (g - Lg[:, None]).abs() + TR)
    t2 = torch.where(kdrow, w * (p - q), torch.zeros_like(p))
    dt2 = torch.where(kdrow, w * (dp + dq + EPS * (p - q).abs()) + EPS * t2.abs(), torch.zeros_like(p))
    d = t1 + t2
    dd = dt1 + dt2 + torch.where(kdrow, EPS * d.abs(), torch.zeros_like(d)) + TINY
    out, allow = torch.zeros(M, Vpad, dtype=F64), torch.zeros(M, Vpad, dtype=F64)
    out[:, :V] = torch.where(active[:, None], d, torch.zeros_like(d))
    allow[:, :V] = torch.where(active[:, None], dd, torch.zeros_like(dd))
    return out, allow


def allow_bf16(d, allow):
    """the allowance of a bf16-stored d: half a bf16 ulp of the value on top (exact zeros stay exact)"""
    return torch.where(allow > 0, allow + 2.0 ** -8 * (d.abs() + allow) + 2.0 ** -134, allow)


def allow_planes(d, allow):
    """the allowance of hi + lo of the (hi | lo) bf16 plane pair"""
    return torch.where(allow > 0, allow + 2.0 ** -16 * (d.abs() + allow) + 2.0 ** -133, allow)


def objective(x, c, u, lse_c, lse_u, s, cf, lab, rows, w, V):
    """sum_m cf_m nll_m + w sum over the loss rows of kd_row, of float64 logits x with their EXACT lse: the function whose gradient
    by x backward() states (cf constant, as in mmtg_loss_bwd)"""
    lse = torch.logsumexp(x[:, :V], 1)
    logp = x[:, :V] - lse[:, None]
    g, _ = teacher_g(c, u, lse_c, lse_u, s, V)
    lq = g - torch.logsumexp(g, 1)[:, None]
    kd = (lq.exp() * (lq - logp)).sum(1)
    nll = -logp.gather(1, lab[:, None])[:, 0]
    return (cf * nll).sum() + w * torch.where(rows, kd, torch.zeros_like(kd)).sum()


# ---------------------------------------------------------------- the cases of tests/test_kd_ops_gpu.py
def padded(V):
    return (V + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def case(V, ldl, ldt, P, L, sbf, tbf):
    """student logits [M, ldl] (normal times 4, a +50 outlier in a loss row, the columns >= V hold 1e4) with their fp32 row lse,
    cfg_ref's teacher pair [M, ldt] with theirs, targets with cfg_ref's planted labels, topic_ids [B, P] and coef [B] (both signs)."""
    cond, uncond, lse_c, lse_u, tg = C.case(V, ldt, P, L, tbf)
    Tt = P + L
    M = B * Tt
    gen = torch.Generator().manual_seed(7000000 + 100000 * int(sbf) + 10 * V + L)
    x = torch.full((M, ldl), 1e4)
    x[:, :V] = torch.randn(M, V, generator=gen) * 4.0
    x[Tt + P, V // 2] += 50.0
    x = x.to(torch.bfloat16 if sbf else torch.float32)
    lse = torch.logsumexp(x[:, :V].to(F64), 1).float()
    topic = torch.randint(0, V, (B, P), generator=gen)
    if P:
        topic[0, 1] = V + 3
    coef = torch.tensor([0.3, -0.7]) / ((L - 1) * B)
    return x, lse, cond, uncond, lse_c, lse_u, tg, topic, coef


def geometries():
    """(V, ldl, ldt, P, L) of every case; the last has fp32 rows of odd strides (student 257, teacher 259: neither row is aligned)"""
    out = [(V, padded(V), padded(V), P, L) for (P, L) in PLS for V in VS]
    out.append((ODD[0], ODD[1], ODD[1] + 2, 3, 5))
    return out
