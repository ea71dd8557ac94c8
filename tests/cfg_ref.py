"""The training side of guidance: a numpy restatement of mmtg_experience_drop's code rule, the float64 reference of mmtg_guided_loss
(the rule in include/mmtg_hip.h), the error bounds of its fp32 evaluation, and a float32 restatement of the kernel's expressions
(csrc/guidance_train.hip: guided_row_kernel, guided_sample_kernel).

Convention (as tests/ul_ref.py): torch on the CPU; the logits come in their storage type and are widened exactly (bf16 -> fp32 is
exact, so the widening adds nothing); the two lse vectors are the fp32 values the kernel is given, widened exactly; a scale is the
fp32 value the kernel receives.

The bounds, derived by counting rounded fp32 operations (EPS = 2^-24 is half an ulp relative; TR = 2^-21 = 8 EPS covers one exponential
STAGE of the kernel: the hardware exponential is within 1 ulp = 2 EPS, the product with log2(e) and the constant's own rounding are
counted with the argument below, the product of a partial sum with the factor is one more EPS; logf is within OpenCL's 3 ulp < TR):

  lc = c - lse_c, lu = u - lse_u     one rounding each: dlc = EPS |lc|, dlu = EPS |lu|
  d = lc - lu                         dd = dlc + dlu + EPS |d|
  g = lu + s d                        dg = dlu + s dd + EPS |s d| + EPS |g|     (the product, the sum; a fused multiply-add rounds once)
      -- s_k AMPLIFIES the error of lc - lu: at s = 7.5 and |lc| = 40 this is 7.5 * 2 * 40 * 2^-24 = 3.6e-5, the largest share
  L(g) = max g + log(sum exp(g - max g)).  L is 1-Lipschitz in the sup norm, so the inputs' errors move it by at most max_v dg.
  The evaluation itself: every element's contribution to the sum is exp(g - running max), later multiplied by exp(old max - new max)
  whenever the running max moves: in the thread (at most one move per slice of 2048 logits and one for its tail element), in the six
  butterfly stages of the wave and the three merges of the four waves.  The maxima only rise, so the arguments of one element's
  stages add up to |a| = max g - g: their roundings (the difference, the product with log2(e), the constant) come to 3 EPS |a| in
  all, and each of the NST = ceil(V / 2048) + 11 stages adds TR.  An element passes at most DEPTH = 8 ceil(V / 2048) + 10 additions of
  positive numbers (its thread's, then the merges'), each (1 + EPS).  With p = softmax(g):
      relS = sum_v p_v (NST TR + 3 EPS |a_v|) + DEPTH EPS          (relative error of the sum S; the row's largest term is exactly 1)
      dL = max_v dg - log(1 - relS) + TR |log S| + EPS |L|          (logf, the last addition)
  nll = L - g[label]                  dnll = dL + dg[label] + EPS |nll|
  sample_ce = (1 / ntok) sum of ntok rows, ANY order: (sum dnll + (ntok - 1) EPS sum |nll|) / ntok + EPS |sample_ce|
  ce = sum_b sample_ce / den:         sum d(sample_ce) / den + (B + 1) EPS sum |sample_ce| / den
"""
import functools
import math

import numpy as np
import torch

EPS = 2.0 ** -24
TR = 2.0 ** -21
F64 = torch.float64
TWO32 = 1 << 32


# ---------------------------------------------------------------- mmtg_experience_drop: the code rule
def hash_u32(seed, idx):
    """The counter hash of csrc/common.h on numpy arrays (uint64 arithmetic masked to 32 bits)."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(int(seed) & 0xFFFFFFFF)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def thresholds(probs):
    """(p_both, p_img, p_txt) -> cumulative (c_both, c_img, c_txt): min(int(p * 2**32), 2**32) in float64, accumulated"""
    out, acc = [], 0
    for p in probs:
        acc += min(int(float(p) * 4294967296.0), TWO32)
        out.append(acc)
    return tuple(out)


def codes(seed, B, thr):
    """int32 [B]: 3 where h < c_both, else 1 where h < c_img, else 2 where h < c_txt, else 0"""
    h = hash_u32(seed, np.arange(B))
    c_both, c_img, c_txt = (np.uint64(t) for t in thr)
    return np.where(h < c_both, 3, np.where(h < c_img, 1, np.where(h < c_txt, 2, 0))).astype(np.int32)


def mix_seed(seed, site):
    """engine.mix_seed, restated"""
    x = (seed ^ (0x9E3779B9 * (site + 1))) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 0x846CA68B) & 0xFFFFFFFF
    return (x ^ (x >> 16)) & 0xFFFFFFFF


def next_step_seed(drop_seed):
    """the step seed Engine.forward draws from the counter it finds"""
    return (drop_seed * 1664525 + 1013904223) & 0xFFFFFFFF


EXP_DROP_SITE = 0x2000
MIXED = (0.25, 0.10, 0.15)
KERNEL_SEEDS = (0, 1, 0xDEADBEEF)


def engine_codes(drop_seed, B, probs):
    """the codes of a forward that finds `drop_seed` in the engine"""
    return codes(mix_seed(next_step_seed(drop_seed), EXP_DROP_SITE), B, thresholds(probs))


# ---------------------------------------------------------------- mmtg_guided_loss: the reference and its bounds
def loss_rows(B, P, L):
    t = torch.arange(B * (P + L)) % (P + L)
    return (t >= P) & (t <= P + L - 2)


def row_labels(targets, P, V):
    """int64 [M]: the label of row (b, t) for the loss rows, targets[b, t + 1 - P] clamped into [0, V); 0 elsewhere"""
    B, L = targets.shape
    Tt = P + L
    lab = torch.zeros(B, Tt, dtype=torch.long)
    lab[:, P:Tt - 1] = targets[:, 1:].clamp(0, V - 1)
    return lab.view(-1)


def reference(c, u, lse_c, lse_u, targets, P, V, scales, batch_den):
    """c, u: [M, >= V] logits in their storage type; lse_c, lse_u: fp32 [M].  Returns float64 tensors: nll [K, M] (0 outside the loss
    rows), sample_ce [K, B], ce [K] and allow_nll, allow_sample, allow_ce; dg_max [K, M] is max_v dg of each row."""
    B, L = targets.shape
    Tt = P + L
    ntok = Tt - 1 - P
    rows = loss_rows(B, P, L)
    lab = row_labels(targets, P, V)
    lc = c[:, :V].to(F64) - lse_c.to(F64)[:, None]
    lu = u[:, :V].to(F64) - lse_u.to(F64)[:, None]
    dlc, dlu = EPS * lc.abs(), EPS * lu.abs()
    d = lc - lu
    dd = dlc + dlu + EPS * d.abs()
    nst = math.ceil(V / 2048) + 11
    depth = 8 * math.ceil(V / 2048) + 10
    den = float(np.float32(batch_den))
    out = {k: [] for k in ("nll", "allow_nll", "sample_ce", "allow_sample", "ce", "allow_ce", "dg_max")}
    for s in scales:
        s = float(np.float32(s))
        g = lu + s * d
        dg = dlu + s * dd + EPS * (s * d).abs() + EPS * g.abs()
        mx = g.max(1).values
        a = g - mx[:, None]
        e = a.exp()
        S = e.sum(1)
        p = e / S[:, None]
        relS = (p * (nst * TR + 3 * EPS * a.abs())).sum(1) + depth * EPS
        Lg = mx + S.log()
        dL = dg.max(1).values - torch.log1p(-relS) + TR * S.log().abs() + EPS * Lg.abs()
        gl = g.gather(1, lab[:, None])[:, 0]
        nll = Lg - gl
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


def reference32(c, u, lse_c, lse_u, targets, P, V, scales, batch_den):
    """The kernel's expressions in float32 (torch on the CPU, its own summation order): nll [K, M], sample_ce [K, B], ce [K]"""
    f = torch.float32
    B, L = targets.shape
    Tt = P + L
    rows = loss_rows(B, P, L)
    lab = row_labels(targets, P, V)
    lc = c[:, :V].to(f) - lse_c[:, None]
    lu = u[:, :V].to(f) - lse_u[:, None]
    nlls, smps, ces = [], [], []
    for s in scales:
        g = lu + torch.tensor(s, dtype=f) * (lc - lu)
        mx = g.max(1).values
        Lg = mx + torch.log(torch.exp2((g - mx[:, None]) * np.float32(1.4426950408889634)).sum(1))
        nll = torch.where(rows, Lg - g.gather(1, lab[:, None])[:, 0], torch.zeros((), dtype=f))
        smp = nll.view(B, Tt)[:, P:Tt - 1].sum(1) / np.float32(Tt - 1 - P)
        nlls.append(nll)
        smps.append(smp)
        ces.append(smp.sum() / np.float32(batch_den))
    return torch.stack(nlls), torch.stack(smps), torch.stack(ces)


def lse_allow(x, V):
    """What an fp32 row log-sum-exp of x[:, :V] (a sum of V positive terms in any order, exponentials and a log within TR each) may
    differ from the exact one by: (V - 1) EPS + 2 TR (1 + |log S|) + EPS |L|, a float64 [M]"""
    x = x[:, :V].to(F64)
    Lx = torch.logsumexp(x, 1)
    S = (x - x.max(1).values[:, None]).exp().sum(1)
    return (V - 1) * EPS + 2 * TR * (1 + S.log().abs()) + EPS * Lx.abs()


def decode_allow(c, u, V, s):
    """What mmtg_decode_guidance's out may differ from the float64 rule by, per row (a float64 [M]): it computes both row
    log-sum-exps itself, each within lse_allow of the exact one, where mmtg_guided_loss is GIVEN them; an error of the lse moves
    every lc (lu) of the row alike, so out moves by at most s dLSE_c + |1 - s| dLSE_u, on top of the dg of the rule's own operations."""
    return s * lse_allow(c, V) + abs(1.0 - s) * lse_allow(u, V)


def plain_ce_allow(x, lse, targets, P, V):
    """What the mean of mmtg_loss_fwd's sample_ce may differ from the EXACT guided cross-entropy at the scale that follows x alone
    (1 for the conditional logits, 0 for the unconditional) by, a float: with the fp32 lse the kernels share, the guided rule gives
    L(x - lse) - (x - lse)[label] = (LSE(x) - lse) + (lse - x[label]), the loss kernel fl(lse - x[label]): they differ by the lse's
    own error (lse_allow) and one rounding per row; then a mean over ntok rows and one over B samples."""
    B, L = targets.shape
    Tt = P + L
    rows = loss_rows(B, P, L)
    lab = row_labels(targets, P, V)
    nll = (lse.to(F64) - x[:, :V].to(F64).gather(1, lab[:, None])[:, 0]).abs()
    per = torch.where(rows, lse_allow(x, V) + EPS * nll, torch.zeros_like(nll))
    mean = torch.where(rows, nll, torch.zeros_like(nll)).sum() / ((Tt - 1 - P) * B)
    return float(per.sum() / ((Tt - 1 - P) * B) + (Tt - 1 - P + B + 2) * EPS * mean)


# ---------------------------------------------------------------- the cases of tests/test_cfg_ops_gpu.py (the CPU file walks the same list)
B = 2
PLS = [(0, 2), (3, 5)]
VS = [1, 2, 7, 8, 9, 160, 255, 256, 257, 13317]
ODD = (255, 257)            # V, ldl of the fp32 case with an odd row stride
KSETS = [[1.5], [0.0, 1.0, 3.0], [0.0, 1.0, 1.5, 3.0, 7.5, 1.0, 0.0, 3.0]]


def padded(V):
    return (V + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def case(V, ldl, P, L, bf):
    """cond, uncond [M, ldl] in their storage type (normal times 4; row 1 of cond carries a +60 and a -60 outlier; the columns >= V
    hold 1e4, which a kernel that read them would show), targets [B, L] with the labels -1, V and V + 5 planted, and the fp32 row lse
    of both (the fp32 rounding of the float64 log-sum-exp of the stored values)."""
    Tt = P + L
    M = B * Tt
    gen = torch.Generator().manual_seed(100000 * int(bf) + 10 * V + L)
    dt = torch.bfloat16 if bf else torch.float32
    mats = []
    for i in range(2):
        x = torch.full((M, ldl), 1e4)
        x[:, :V] = torch.randn(M, V, generator=gen) * 4.0
        if i == 0:
            m = P if L > 2 else Tt + P          # a loss row
            x[m, 0] += 60.0
            x[m, V - 1] -= 60.0
        mats.append(x.to(dt))
    tg = torch.randint(0, V, (B, L), generator=gen)
    if L == 2:
        tg[0, 1], tg[1, 1] = -1, V + 5
    else:
        tg[0, 1], tg[0, 3], tg[1, 2] = -1, V, V + 5
        tg[1, 0] = V + 9                        # (column 0 is never a label)
    lse = [torch.logsumexp(x[:, :V].to(F64), 1).float() for x in mats]
    return mats[0], mats[1], lse[0], lse[1], tg


def geometries():
    """(V, ldl, P, L, bf) of every case"""
    out = [(V, padded(V), P, L, bf) for bf in (False, True) for (P, L) in PLS for V in VS]
    out.append((ODD[0], ODD[1], 3, 5, False))
    return out
