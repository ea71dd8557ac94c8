"""The causal attention kernels against a float64 restatement, at their tile, chunk and mask edges (csrc/attention.hip).

tests/test_ops_gpu.py checks them against fp32 torch with one absolute bound per tensor, on randn inputs and one mask pattern in
which key 0 is always kept.  Here every case hands mmtg_attn_fwd / mmtg_attn_bwd inputs already rounded to their storage type
(mmtg_attn_fwd_x3 / mmtg_attn_bwd_x3: values that are the sum of a (hi | lo) plane pair) and compares every element of what
they wrote with the same operation restated in float64 on the CPU, under a bound built from the reference's own quantities for
that element:

  1. the case table: kernel families (bf16 whole-head MT = 256 / 512, bf16 tiled, fp32 tiled, split precision), geometries, T
     values, mask patterns (left padding and empty rows included: query rows without a visible key) and value patterns (sharp,
     ramps, identical keys, loud padding);
  2. the float64 reference and the per-element bounds, each term derived where it is added;
  3. the rounding model: a CPU restatement that rounds where the kernels round (float64 otherwise, float32 for the fp32 family); it
     must pass every bound on every case, and with one defect planted it must be rejected -- both without a GPU;
  4. the kernel cases: out, lse, d(qkv), the exact zeros, the three forms of the fused bias gradient, delta_ready, and sentinels
     around every buffer the kernels read or write;
  5. metamorphic checks of the whole-head path, bit for bit;
  6. dropout: the keep matrix of every (b, h) recovered with unit-vector probes, forward and backward against the reference that
     uses it, the matrices' independence and their kept fraction;
  7. the kernels behind MMTG_ATTN_KV2 / MMTG_ATTN_KV_NW / MMTG_ATTN_TILED (read once per process), each in a child process.

Case count: the table holds 881 cases (295 + 137 + 39 + 251 + 159 over the five families): every T of a family at B = 2, nH = 3
and eight (family, geometry, T) extras, each over the ten mask patterns that fit with randn values, plus the five value patterns
over four masks at the T subset of each family.  They run as 75 kernel tests (one per family, geometry, T and "masks" / "values"
group), beside 18 dropout cases, 6 metamorphic tests and 5 child processes of 115 cases each.  One term of the bounds rests on a
measured yardstick, the error of the exponential (EXP_YARD, test_exp_yardstick); lse and the logarithm are bounded by derivation
(section 2).  docs/experiments.md records the yardstick and the kernels' margins.
"""
import functools
import hashlib
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # (section 7 runs this file as a script in a child process)
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402
import torch  # noqa: E402

from mmtg_amd import hip  # noqa: E402

gpu = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 1234.0                # sentinel around every output (exact in bf16)
PAD = 64                     # elements in front of and behind every buffer: 16-byte aligned for every type used
DH = 64


# =====================================================================================================================
# 1. the case table
# =====================================================================================================================
# up: relative rounding of P and dS as matrix-core operands, the unit roundoff of the type: 2^-8 for bf16 (8 significant bits: half
# an ulp is 2^-9 of the value only at the top of a binade and 2^-8 at its bottom, and the unnormalised P the kernels round sits
# anywhere in its binade), 2^-24 for fp32; um: of one product of an operand pair (bf16 products are exact in fp32; the fp32 matrix
# core rounds each product and sum, taken as 2^-23 per term).  A STORED output is allowed exactly half an ulp of its type at the
# largest magnitude the other terms leave it (_half_ulp): between 2^-9 and 2^-8 of the value for bf16.
FAM = {
    "wh256": dict(dtype=BF, whole=True, up=2.0 ** -8, um=0.0,
                  Ts=[1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 236, 255, 256], sub=[17, 33, 65, 129, 236, 256]),
    "wh512": dict(dtype=BF, whole=True, up=2.0 ** -8, um=0.0,
                  Ts=[257, 383, 384, 385, 497, 511, 512], sub=[257, 385, 512]),
    "tiled16": dict(dtype=BF, whole=False, up=2.0 ** -8, um=0.0, Ts=[513, 1024], sub=[513]),
    "tiled32": dict(dtype=F32, whole=False, up=2.0 ** -24, um=2.0 ** -23,
                    Ts=[1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 236, 257, 513], sub=[33, 65, 129, 236, 257, 513]),
    # split precision: every operand a (hi | lo) bf16 pair.  hi is within 2^-8 |x| of x and lo within 2^-8 of what is left, so a pair
    # is within 2^-16 |x|, and 2^-17 (the figure tests/test_x3_gpu.py already holds the stored pairs to) wherever |lo| <= 2^-9 |x|;
    # up takes the 2^-16.  The three-pass product leaves out lo x lo, at most 2^-8 2^-8 of the product: um = 2^-16; and it
    # accumulates 3 x 64 terms where the others accumulate 64 (acc = 3).
    "x3": dict(dtype=F32, whole=False, up=2.0 ** -16, um=2.0 ** -16, acc=3, Ts=[1, 63, 64, 65, 127, 128, 129, 236, 257], sub=[65, 129, 236, 257]),
}
# The one term of the bounds that is measured, not derived: the relative error of the exponential (the hardware exp2 of the bf16
# kernels, expf in the fp32 family).  EXP_YARD is the largest error of float32 exp2 / exp on the CPU against float64 over the
# table's own exponents (test_exp_yardstick prints it; docs/experiments.md records it), and the kernels are allowed EXP_FACTOR
# times it, as LSE_YARD / LSE_FACTOR of tests/test_train_ops_gpu.py.
EXP_YARD = 7.2e-8
EXP_FACTOR = 4.0
BASE = (2, 3)
EXTRA_GEOM = [("wh256", (1, 1), 17), ("wh256", (1, 1), 236), ("wh256", (3, 2), 17), ("wh256", (3, 2), 236), ("wh256", (1, 12), 33),
              ("tiled32", (3, 2), 17), ("tiled32", (1, 12), 33), ("wh512", (1, 1), 385)]
MASKS = ["ones", "rpad", "rpad2", "holes", "lpad1", "lpad16", "lpad17", "lpad40", "zero-row", "key0"]
VALUES = ["sharp", "ramp-up", "ramp-down", "same-keys", "loud"]
VALUE_MASKS = ["ones", "holes", "lpad17", "rpad"]


def _keep(mask, B, T):
    """[B, T] int32, or None where the pattern does not fit T"""
    k = torch.ones(B, T, dtype=torch.int32)
    if mask == "ones":
        return k
    if mask in ("rpad", "rpad2"):          # right padding as the data makes it: kept lengths T - 1, T - 17, 1 over the batch rows
        lens = [T - 1, T - 17, 1] if mask == "rpad" else [1, T - 1, T - 17]
        lens = [n for n in lens if 1 <= n < T]
        if not lens:
            return None
        for b in range(B):
            k[b, lens[b % len(lens)]:] = 0
        return k
    if mask == "holes":                    # the pattern of test_attention
        if T < 16:
            return None
        k[0, 9:15] = 0
        k[B - 1, 20:41] = 0
        k[B - 1, T - 3:] = 0
        return k
    if mask.startswith("lpad"):            # rows without a visible key, then ordinary rows behind them; the other batch rows plain
        n = int(mask[4:])
        if n >= T:
            return None
        k[0, :n] = 0
        return k
    if mask == "zero-row":
        k[0] = 0
        return k
    if mask == "key0":
        k[:, 1:] = 0
        return k
    raise KeyError(mask)


def _pair(x):
    """fp32 x as its (hi | lo) bf16 pair stores it: hi + lo, exact in fp32"""
    x = x.float()
    hi = x.to(BF).float()
    return hi + (x - hi).to(BF).float()


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=6)
def _case(fam, geom, T, mask, values):
    """inputs as stored: qkv [B, T, 3D], dout [B, T, D] in the family's storage type, keep [B, T]; None where the mask does not fit"""
    B, nH = geom
    D = nH * DH
    keep = _keep(mask, B, T)
    if keep is None:
        return None
    seed = 7919 * T + 31 * B + nH + 1009 * MASKS.index(mask)
    qkv = _randn((B, T, 3 * D), seed)
    dout = _randn((B, T, D), seed + 1)
    q, k, v = (qkv[..., i * D:(i + 1) * D].view(B, T, nH, DH) for i in range(3))      # views into qkv
    j = torch.arange(T, dtype=torch.float32)
    if values == "sharp":
        # scores q.k / 8 of N(0, s^2) entries have standard deviation s^2: s = sqrt(8) gives about 8 -- a near one-hot softmax
        q *= math.sqrt(8.0)
        k *= math.sqrt(8.0)
    elif values in ("ramp-up", "ramp-down"):
        # key j's score rises (falls) by about 0.25 per key on top of unit noise: the running maximum rises at every 64-key chunk
        # by about 16 (or the first key wins and every later chunk rescales by nothing)
        u = _randn((B, 1, nH, DH), seed + 2)
        u = u / u.norm(dim=-1, keepdim=True)
        q += 8.0 * u
        k += (0.25 if values == "ramp-up" else -0.25) * j.view(1, T, 1, 1) * u
    elif values == "same-keys":
        k[:] = k[:, :1].clone()                   # uniform attention over the visible keys: out = their running mean
    elif values == "loud":
        # every padded position 64 times louder, and the first padded key of each batch row = 32 q[T - 1]: its unmasked score
        # against the last query is far above that row's lse.  Nothing of this may reach a kept position.
        pad = (keep == 0)
        if not bool(pad.any()):
            return None
        qkv[pad] *= 64.0
        dout[pad] *= 64.0
        for b in range(B):
            idx = pad[b].nonzero()
            if len(idx):
                k[b, int(idx[0])] = 32.0 * q[b, T - 1]
    elif values != "randn":
        raise KeyError(values)
    if fam == "x3":
        return _pair(qkv), _pair(dout), keep
    dtype = FAM[fam]["dtype"]
    return qkv.to(dtype), dout.to(dtype), keep


def _split(qkv, dout, nH, dt=F64):
    """q, k, v, dO as [B, nH, T, 64] in dt"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (qkv[..., i * D:(i + 1) * D].to(dt).view(B, T, nH, DH).transpose(1, 2) for i in range(3))
    return q, k, v, dout.to(dt).view(B, T, nH, DH).transpose(1, 2)


def _merge(x):
    """[B, nH, T, 64] -> [B, T, D]"""
    B, nH, T, _ = x.shape
    return x.transpose(1, 2).reshape(B, T, nH * DH)


def _visible(keep):
    """[B, 1, T, T]: key <= query and keep[b, key] != 0"""
    T = keep.shape[1]
    return (torch.tril(torch.ones(T, T, dtype=torch.bool))[None] & (keep != 0)[:, None, :])[:, None]


# =====================================================================================================================
# 2. the float64 reference and the bounds
# =====================================================================================================================
def _reference(qkv, dout, keep, nH, Mc=None):
    """Mc: None, or [B, nH, T, T] float64 = dropout keep matrix times the family's scale.  A query row with no visible key has
    p = 0, out = 0, lse = -inf, contributes to no gradient, and its own dQ is 0 (the forward kernels' contract)."""
    q, k, v, dO = _split(qkv, dout, nH)
    vis = _visible(keep)
    S = q @ k.transpose(-1, -2) / 8.0
    Sm = S.masked_fill(~vis, -INF)
    has = vis.any(-1).expand(S.shape[:3])
    m = Sm.max(-1).values
    m0 = torch.where(has, m, torch.zeros_like(m))
    lse = torch.where(has, m0 + (Sm - m0[..., None]).exp().sum(-1).log(), torch.full_like(m, -INF))
    lse0 = torch.where(has, lse, torch.zeros_like(lse))
    P = (Sm - lse0[..., None]).exp()
    Pd = P if Mc is None else P * Mc
    out = Pd @ v
    dPd = dO @ v.transpose(-1, -2)
    dP = dPd if Mc is None else dPd * Mc
    delta = (dO * out).sum(-1)
    dS = P * (dP - delta[..., None])
    r = dict(q=q, k=k, v=v, dO=dO, vis=vis, has=has, S=S, lse=lse, lse0=lse0, P=P, Pd=Pd, out=out, dP=dP, delta=delta, dS=dS,
             Mc=Mc, keep=keep, dQ=dS @ k / 8.0, dK=dS.transpose(-1, -2) @ q / 8.0, dV=Pd.transpose(-1, -2) @ dO)
    return r


def _half_ulp(x, dtype):
    """half the spacing of dtype at magnitude x >= 0 (float64): x = m 2^e with m in [0.5, 1) has spacing 2^(e - bits)"""
    if dtype == "pair":               # a (hi | lo) bf16 pair: see FAM["x3"]
        return 2.0 ** -16 * x
    _, e = torch.frexp(x)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - (9 if dtype == BF else 25)), torch.zeros_like(x))


def _bounds(r, fam):
    """Per-element allowances for out, lse [B, nH, T, ..] and dQ, dK, dV [B, nH, T, 64], from the reference's quantities.

    Scores.  s = q.k / 8 is a 64-term sum accumulated in fp32: each partial sum is at most A = sum_d |q_d k_d| / 8, so the sum is
    within 64 2^-24 A = 2^-18 A (+ um A for rounded products).  The exponent x = s log2 e - (max or lse) log2 e takes two more
    roundings at magnitudes |s| and |s| + |lse|, the constant log2 e one of 2^-24 |s|, and the hardware exp2 (expf in the fp32
    family) is allowed Ee = EXP_FACTOR EXP_YARD relative, the measured yardstick above.  An absolute error e of x in log2 units moves p by e ln 2 relative, which takes
    the log2 e out again: Es = (2^-18 + um) A + 2^-22 (|s| + L) + Ee relative on p, with L = |lse| + log(T + 1) >= |max|.
    lse = max + log(l): the sum l carries the P-weighted mean Ebar of Es and its own fp32 accumulation over at most T + 64
    positive terms (accT = (T + 64) 2^-24, which also covers the handful of scalings at the end); the logarithm, the product with
    1 / log2 e and the final sum are rounded at magnitude L: allow_lse = Ebar + accT + 2^-22 (L + 1).
    out = sum_j p_j v_j / l: each p_j is off by Es + Ebar + accT relative (its own exponent and the normaliser), rounded as an
    operand (up), each product by um, the accumulation by accT of the sum of magnitudes; then the storage rounding, half an ulp.
    Second-order products of these terms are covered by the factor 1 + 2^-6 (no first-order term here exceeds 2^-7).
    fp32 flushes results below 2^-126 that float64 keeps: 1e-30 absolute.

    Backward.  p is recomputed as exp2(x - lse_stored): Rb = Es + allow_lse + 2^-23 |lse| (fp32 storage of lse) + 2^-22.
    delta is taken from the STORED out: e_delta = sum_d |dO_d| allow_out_d + 2^-18 sum_d |dO_d out_d| (64-term fp32 sum).
    dP = dO.v is a 64-term sum like the scores: (2^-18 + um) sum_d |dO_d v_d|, times the dropout factor.
    dS = p (dP - delta): e_dS = P (Rb |dP - delta| + e_dP + e_delta + 2^-22 (|dP| + |delta|)) + up |dS| as an operand.
    dQ = dS K / 8, dK = dS^T Q / 8: e_dS (+ (um + accT) |dS| for products and accumulation -- the fp32 atomics of the tiled dQ are
    fp32 sums in some order, inside accT) against |K| / 8 or |Q| / 8; dV = Pd^T dO with p off by Rb + up + um + accT relative.
    Each gradient is then rounded to its storage (half an ulp)."""
    f = FAM[fam]
    up, um = f["up"], f["um"]
    hu = lambda x: _half_ulp(x, f["dtype"])                                     # out (fp32 in the split-precision family)
    hg = lambda x: _half_ulp(x, "pair" if fam == "x3" else f["dtype"])          # the gradients (a plane pair there)
    ea = f.get("acc", 1) * 2.0 ** -18                                           # a 64-term (3 x 64-term) fp32 accumulation
    T = r["S"].shape[-1]
    absq, absk, absv, absdO = (r[n].abs() for n in ("q", "k", "v", "dO"))
    accT = (T + 64) * 2.0 ** -24
    so = 1.0 + 2.0 ** -6
    L = (r["lse0"].abs() + math.log(T + 1.0))[..., None]
    Es = (ea + um) * (absq @ absk.transpose(-1, -2)) / 8.0 + 2.0 ** -22 * (r["S"].abs() + L) + EXP_FACTOR * EXP_YARD
    P, Pd = r["P"], r["Pd"]
    Ebar = (P * Es).sum(-1, keepdim=True)
    a_lse = (Ebar + accT + 2.0 ** -22 * (L + 1.0)).squeeze(-1)
    w_out = so * ((Pd * (Es + Ebar + 2 * accT + up + um)) @ absv)
    a_out = w_out + hu(r["out"].abs() + w_out) + 1e-30
    Rb = Es + a_lse[..., None] + 2.0 ** -23 * r["lse0"].abs()[..., None] + 2.0 ** -22
    e_delta = ((absdO * a_out).sum(-1) + 2.0 ** -18 * (absdO * r["out"].abs()).sum(-1))[..., None]
    mc = 1.0 if r["Mc"] is None else r["Mc"]
    e_dP = (ea + um) * (absdO @ absv.transpose(-1, -2)) * mc
    dS = r["dS"]
    e_dS = so * (P * (Rb * (r["dP"] - r["delta"][..., None]).abs() + e_dP + e_delta
                      + 2.0 ** -22 * (r["dP"].abs() + r["delta"].abs()[..., None])) + (up + um + accT) * dS.abs())
    w_dq = e_dS @ absk / 8.0
    w_dk = e_dS.transpose(-1, -2) @ absq / 8.0
    w_dv = so * ((Pd * (Rb + up + um + 2 * accT)).transpose(-1, -2) @ absdO)
    return dict(lse=a_lse, out=a_out,
                dQ=w_dq + hg(r["dQ"].abs() + w_dq) + 1e-30,
                dK=w_dk + hg(r["dK"].abs() + w_dk) + 1e-30,
                dV=w_dv + hg(r["dV"].abs() + w_dv) + 1e-30)


QUANT = ["out", "lse", "dQ", "dK", "dV"]


def _judge(name, r, a, got, quants=QUANT):
    """got: out, dQ, dK, dV as [B, nH, T, 64], lse [B, nH, T] (CPU).  Returns (worst err / allowed per quantity, failures): the
    bounds element by element, and the values that must be exact -- lse = -inf and out = 0 of a row without a visible key, its
    dQ = 0, dK = dV = 0 of a key that no query sees (a padded one)."""
    worst, fails = {}, []
    has = r["has"]
    unseen = (r["keep"] == 0)[:, None, :].expand(has.shape)
    for qn in quants:
        g, ref, al = got[qn].double(), r[qn], a[qn]
        if qn == "lse":
            same = (g == ref) & ~has                       # -inf where the reference says so: exact, and out of the subtraction
            if not bool((g[~has] == -INF).all()):
                fails.append("%s lse: a row without a visible key must have lse = -inf, got %s" % (name, g[~has][:4].tolist()))
            err = torch.where(same | ~has, torch.zeros_like(g), (g - ref).abs())
        else:
            err = (g - ref).abs()
        ratio = (err / al).nan_to_num(nan=INF)
        worst[qn] = float(ratio.max()) if ratio.numel() else 0.0
        if worst[qn] > 1.0:
            i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
            fails.append("%s %s: %d/%d outside the bound, worst at %s: got %.9g, ref %.9g, allowed %.3g (err/allowed %.3g)" % (
                name, qn, int((ratio > 1).sum()), ratio.numel(), i, float(g[i]), float(ref[i]), float(al[i]), worst[qn]))
        zero = {"out": ~has, "dQ": ~has, "dK": unseen, "dV": unseen}.get(qn)
        if zero is not None and not bool((g[zero] == 0).all()):
            z = g[zero]
            fails.append("%s %s: %d of %d elements that must be exactly 0 are not (first %s)" % (
                name, qn, int((z != 0).sum()), z.numel(), z[(z != 0) | z.isnan()][:4].tolist()))
    return worst, fails


# =====================================================================================================================
# 3. the rounding model
# =====================================================================================================================
def _model(fam, qkv, dout, keep, nH, Mc=None, defect=None, dt=F64):
    """The kernels' arithmetic restated on the CPU in dt, rounding where they round: inputs as stored, the online softmax over
    64-key chunks with the unnormalised P rounded to the operand type before P V, out and lse to their storage, the backward's P
    from the stored lse, delta from the stored out, dS and P rounded as operands, the gradients to their storage.  defect plants one
    of the mistakes of test_planted_defects_are_rejected."""
    f = FAM[fam]
    st = f["dtype"]
    rnd = (lambda x: x.to(st).to(dt))                    # operands and stored gradients
    rnd_o = rnd                                          # the stored out
    if fam == "x3":
        rnd, rnd_o = (lambda x: _pair(x).to(dt)), (lambda x: x.float().to(dt))
    q, k, v, dO = _split(qkv, dout, nH, dt)
    B, _, T, _ = q.shape
    vis = _visible(keep).clone()
    if defect == "causal-lt":              # `<` for `<=` in the last 16-key tile on the diagonal
        t0 = (T - 1) // 16 * 16
        i = torch.arange(t0, T)
        vis[:, :, i, i] = False
    elif defect == "padded-kept":          # the first padded key of batch row 0 (else of the last) treated as kept
        b = 0 if bool((keep[0] == 0).any()) else B - 1
        j = int((keep[b] == 0).nonzero()[0])
        vis[b, :, j:, j] = True
    elif defect == "last-key":             # key T - 1 dropped
        vis[:, :, T - 1, T - 1] = False
    vis = vis.expand(B, nH, T, T)
    S = q @ k.transpose(-1, -2) / 8.0
    Sm = S.masked_fill(~vis, -INF)
    M = None if Mc is None else (Mc != 0).to(dt)
    c = 1.0 if Mc is None else float(Mc.max())
    if defect == "mask-00":                # the dropout mask of (b, h) = (0, 0) for every head
        M = M[:1, :1].expand(B, nH, T, T)
    cin = 1.0 if f["whole"] else c         # the tiled kernels scale P before rounding it, the whole-head ones after the sums
    m = torch.full((B, nH, T), -INF, dtype=dt)
    l = torch.zeros(B, nH, T, dtype=dt)
    o = torch.zeros(B, nH, T, DH, dtype=dt)
    for ci, j0 in enumerate(range(0, T, 64)):
        sc = Sm[..., j0:j0 + 64]
        m_new = torch.maximum(m, sc.max(-1).values)
        m_use = torch.where(m_new == -INF, torch.zeros_like(m_new), m_new)
        alpha = (m - m_use).exp()
        if defect == "alpha" and ci == 1:  # the running-maximum rescale skipped for the second chunk
            alpha = torch.ones_like(alpha)
        p = (sc - m_use[..., None]).exp()
        l = l * alpha + p.sum(-1)
        if M is not None:
            p = p * M[..., j0:j0 + 64] * cin
        o = o * alpha[..., None] + rnd(p) @ v[:, :, j0:j0 + 64]
        m = m_new
    ok = l > 0
    inv = torch.where(ok, (c / cin) / l, torch.zeros_like(l))
    out = rnd_o(o * inv[..., None])
    lse = torch.where(ok, m + l.log(), torch.full_like(l, -INF)).float().to(dt)
    # backward
    lse_b = torch.where(lse == -INF, torch.full_like(lse, INF), lse)
    P = (Sm - lse_b[..., None]).exp()
    dP = dO @ v.transpose(-1, -2)
    Pm = P
    if M is not None:
        dP = dP * M * c
        Pm = P * M * cin
    delta = (dO * out).sum(-1)
    if defect == "delta-head":             # delta read from head h + 1
        delta = delta.roll(-1, 1)
    dS = rnd(P * (dP - delta[..., None]) / 8.0)
    dSk, Pk = dS, rnd(Pm)
    if defect == "last-qblock":            # the last 32-query block left out of dK / dV
        q0 = (T - 1) // 32 * 32
        dSk, Pk = dS.clone(), Pk.clone()
        dSk[:, :, q0:] = 0
        Pk[:, :, q0:] = 0
    dQ = rnd(dS @ k)
    dK = rnd(dSk.transpose(-1, -2) @ q)
    dV = rnd((Pk.transpose(-1, -2) @ dO) * (c / cin))
    return dict(out=out, lse=lse, dQ=dQ, dK=dK, dV=dV)


def _table(fam):
    """(geometry, T, mask, values) of every case of a family"""
    f = FAM[fam]
    cases = [(BASE, T, mk, "randn") for T in f["Ts"] for mk in MASKS]
    cases += [(g, T, mk, "randn") for (fm, g, T) in EXTRA_GEOM if fm == fam for mk in MASKS]
    cases += [(BASE, T, mk, vl) for T in f["sub"] for vl in VALUES for mk in VALUE_MASKS]
    return [cs for cs in cases if _case(fam, *cs) is not None]


@functools.lru_cache(maxsize=4)
def _ref_of(fam, geom, T, mask, values):
    qkv, dout, keep = _case(fam, geom, T, mask, values)
    r = _reference(qkv, dout, keep, geom[1])
    return r, _bounds(r, fam)


def _name(fam, geom, T, mask, values):
    return "%s B=%d nH=%d T=%d %s %s" % ((fam,) + tuple(geom) + (T, mask, values))


@pytest.mark.parametrize("fam", list(FAM))
def test_rounding_model_passes_every_bound(fam):
    """section 3: a bound the restatement cannot meet is a wrong derivation, not a kernel bug.  The fp32 family is run in
    float32 (torch's CPU products: another summation order than the kernel's, the same worst-case bound)."""
    dt = F32 if FAM[fam]["dtype"] == F32 else F64
    worst = dict.fromkeys(QUANT, 0.0)
    for cs in _table(fam):
        qkv, dout, keep = _case(fam, *cs)
        r, a = _ref_of(fam, *cs)
        w, fails = _judge(_name(fam, *cs), r, a, _model(fam, qkv, dout, keep, cs[0][1], dt=dt))
        assert not fails, "\n".join(fails)
        worst = {qn: max(worst[qn], w[qn]) for qn in QUANT}
    print("rounding model, worst err / allowed over the table of %s:" % fam, worst)


def _cpu_mask(B, nH, T, p, seed):
    """a stand-in for a recovered keep matrix: independent bits, times the scale 1 / (1 - p)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, nH, T, T, generator=g) >= p).double() / (1.0 - p)


DEFECTS = {
    # defect: the cases offered (family, geometry, T, mask, values); at least one must reject it
    "causal-lt": [("wh256", BASE, 17, "ones", "randn"), ("wh256", BASE, 65, "ones", "ramp-up")],
    "padded-kept": [("wh256", BASE, 33, "holes", "randn"), ("wh256", BASE, 236, "rpad", "randn")],
    "last-key": [("wh256", BASE, 17, "ones", "randn"), ("tiled16", BASE, 513, "ones", "randn")],
    "alpha": [("wh256", BASE, 65, "ones", "ramp-up"), ("wh256", BASE, 129, "ones", "randn")],
    "delta-head": [("wh256", BASE, 17, "ones", "randn"), ("wh256", (3, 2), 236, "ones", "randn")],
    "last-qblock": [("wh256", BASE, 33, "ones", "randn"), ("wh256", BASE, 236, "holes", "randn")],
    "mask-00": [("wh256", BASE, 64, "ones", "randn")],
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_are_rejected(defect):
    """section 3: the model with one defect planted must fall outside the bounds (or miss an exact value) on a case of the table"""
    rejected = []
    for fam, geom, T, mask, values in DEFECTS[defect]:
        qkv, dout, keep = _case(fam, geom, T, mask, values)
        Mc = _cpu_mask(geom[0], geom[1], T, 0.3, T) if defect == "mask-00" else None
        r = _reference(qkv, dout, keep, geom[1], Mc)
        a = _bounds(r, fam)
        nm = _name(fam, geom, T, mask, values)
        _, clean = _judge(nm, r, a, _model(fam, qkv, dout, keep, geom[1], Mc))
        assert not clean, "the model without a defect must pass: " + "\n".join(clean)
        w, fails = _judge(nm, r, a, _model(fam, qkv, dout, keep, geom[1], Mc, defect=defect))
        if fails:
            rejected.append((nm, {qn: round(x, 1) for qn, x in w.items() if x > 1}))
    print("defect %s rejected by:" % defect, rejected)
    assert rejected, "no case rejects the defect " + defect
    assert rejected[0][0] == _name(*DEFECTS[defect][0]), "the first case listed is the one meant to reject it"


YARD_CASES = [(fam, BASE, T, "holes", vl) for fam, T in (("wh256", 236), ("wh512", 512), ("tiled32", 236)) for vl in ["randn"] + VALUES]


def test_exp_yardstick():
    """section 2's one measured term: float32 exp2 (and exp, which the fp32 family calls) on the CPU against float64, over the
    exponents (s - lse) log2 e of every visible (query, key) pair of the cases above whose result is a normal fp32 number.  The
    figure it prints is EXP_YARD's source; the assertion is against the allowance the kernels get, not against the figure."""
    worst = 0.0
    for fam, geom, T, mask, values in YARD_CASES:
        r, _ = _ref_of(fam, geom, T, mask, values)
        x = ((r["S"] - r["lse0"][..., None]) * math.log2(math.e))[r["vis"].expand_as(r["S"])].float()
        x = x[x > -126.0]
        y = x / math.log2(math.e)
        for fn, z in ((torch.exp2, x), (torch.exp, y[y > -87.0])):
            ref = fn(z.double())
            worst = max(worst, float(((fn(z).double() - ref).abs() / ref).max()))
    print("float32 exp2 / exp against float64, largest relative error over %d cases: %.3e (EXP_YARD %.3e)" % (len(YARD_CASES), worst, EXP_YARD))
    assert worst <= EXP_FACTOR * EXP_YARD, worst


def test_loud_padding_is_the_overflow_case():
    """the loud pattern's purpose, on the float64 reference: some (query, padded key <= query) pair of a row WITH a visible key has
    (s - lse) log2 e > 128, so an unmasked exp2 of it overflows fp32 -- and the padded positions' gradients are exactly 0 in the
    reference, the kept ones' values untouched by what the padded positions hold"""
    n = 0
    for fam in FAM:
        for cs in _table(fam):
            if cs[3] != "loud" or cs[1] > 600:
                continue
            r, _ = _ref_of(fam, *cs)
            pad = (r["keep"] == 0)[:, None, None, :]
            causal = torch.tril(torch.ones(cs[1], cs[1], dtype=torch.bool))
            x = (r["S"] - r["lse0"][..., None]) * math.log2(math.e)
            hit = (x > 128) & pad & causal & r["has"][..., None]
            assert bool(hit.any()), _name(fam, *cs)
            unseen = (r["keep"] == 0)[:, None, :, None].expand_as(r["dK"])
            assert bool((r["dK"][unseen] == 0).all()) and bool((r["dV"][unseen] == 0).all())
            n += 1
    assert n >= 12, n


# =====================================================================================================================
# 4. the kernel cases
# =====================================================================================================================
def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


class _Framed:
    """a device buffer of the given shape inside a larger allocation: PAD elements of `outside` in front and behind"""

    def __init__(self, shape, dtype, inside, outside, src=None):
        n = math.prod(shape)
        self.flat = torch.full((n + 2 * PAD,), outside, dtype=dtype, device=DEV)
        self.t = self.flat[PAD:PAD + n].view(shape)
        if src is not None:
            self.t.copy_(src)
        else:
            self.t.fill_(inside)
        self.edge = torch.cat([self.flat[:PAD], self.flat[PAD + n:]]).clone()
        assert self.t.data_ptr() % 16 == 0

    def untouched(self):
        now = torch.cat([self.flat[:PAD], self.flat[-PAD:]])
        return torch.equal(_bits(now), _bits(self.edge))


def _framed_planes(rows, cols, inside, outside, src=None):
    """a (hi | lo) plane pair [2, rows, cols] inside a larger allocation; src: fp32 [rows, cols] on the CPU, split on the device"""
    fr = _Framed((2, rows, cols), BF, inside, outside)
    pl = hip.Planes(fr.t, rows, cols)
    if src is not None:
        hip.split_planes(src.to(DEV).contiguous(), rows, cols, pl)
        assert torch.equal((fr.t[0].float() + fr.t[1].float()).cpu(), src), "the device's plane pair of a value that is a pair's sum must be that value"
        fr.edge = torch.cat([fr.flat[:PAD], fr.flat[-PAD:]]).clone()
    return fr, pl


def _run_x3(qkv, dout, keep, nH, drop_p, seed, forms):
    """_run for mmtg_attn_fwd_x3 / mmtg_attn_bwd_x3: inputs and d(qkv) as plane pairs, out fp32.  d(qkv) comes back as hi + lo."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    fails = []
    fq, qp = _framed_planes(B * T, 3 * D, 0, NAN, qkv.view(B * T, 3 * D))
    fd, dp = _framed_planes(B * T, D, 0, NAN, dout.view(B * T, D))
    fk = _Framed((B, T), torch.int32, 0, 7, keep)
    fo = _Framed((B * T, D), F32, NAN, SENT)
    fl = _Framed((B, nH, T), F32, NAN, SENT)
    kw = dict(drop_p=drop_p, drop_seed=seed)
    hip.attn_fwd_x3(qp, fk.t, fo.t, None, fl.t, B, T, nH, DH, **kw)

    def bwd(with_rows, delta=None):
        fg, gp = _framed_planes(B * T, 3 * D, NAN, SENT)
        fdel = _Framed((B * T, nH), F32, NAN, SENT, delta)
        fdq = _Framed((hip.attn_bwd_x3_dq_floats(B, T, D),), F32, NAN, SENT)
        fws = _Framed((hip.attn_bwd_x3_ws(B, T, D),), F32, NAN, SENT)
        dbias = torch.full((3 * D,), 0.5, device=DEV)
        hip.attn_bwd_x3(qp, fk.t, fo.t, dp, fl.t, fdel.t, fdq.t, gp, B, T, nH, DH, dbias=None if with_rows else dbias, dbias_ws=fws.t,
                        delta_ready=delta is not None, **kw)
        if with_rows:          # the partial rows left for the batched column sums: k and v parts from the key-block rows, q from the band rows
            nkv, nq = B * (-(-T // 128)), -(-(B * T) // 16)
            hip.colsum_batch([(fws.t.data_ptr() + 4 * D, dbias.data_ptr() + 4 * D, 3 * D, nkv, 2 * D),
                              (fws.t.data_ptr() + 4 * nkv * 3 * D, dbias.data_ptr(), D, nq, D)])
        for nm, fr in (("dqkv planes", fg), ("delta", fdel), ("dq32", fdq), ("dbias_ws", fws)):
            if not fr.untouched():
                fails.append("%s: written outside the buffer" % nm)
        return fg.t.cpu(), (fg.t[0].float() + fg.t[1].float()).cpu().view(B, T, 3 * D), fdel.t.cpu(), dbias.cpu()

    gbits, dqkv, delta, dbias = bwd(False)
    for nm, fr in (("qkv planes", fq), ("dout planes", fd), ("keep", fk), ("out", fo), ("lse", fl)):
        if not fr.untouched():
            fails.append("%s: written outside the buffer" % nm)
    res = dict(out=fo.t.cpu().view(B, T, D), lse=fl.t.cpu(), dqkv=dqkv, delta=delta)
    if bool(delta.isnan().any()):
        fails.append("delta: %d elements NaN or never written" % int(delta.isnan().sum()))
    if not forms:
        return res, fails
    # the bias gradient: the kernels sum the fp32 values they then split, so against the column sums of the STORED pairs each term
    # may differ by the pair's residual, 2^-16 of its magnitude, on top of the n 2^-24 of an fp32 sum of n = B T terms
    g64 = dqkv.double().view(B * T, 3 * D)
    bref, ball = 0.5 + g64.sum(0), (B * T * 2.0 ** -24 + 2.0 ** -16) * (0.5 + g64.abs().sum(0)) + 1e-30
    # no atomics anywhere in this backward: every form and every repeat gives the same bits
    for form, (g2, _, d2, db) in (("one call", (gbits, None, delta, dbias)), ("partial rows", bwd(True)), ("delta_ready", bwd(False, delta=delta))):
        if not (torch.equal(_bits(g2), _bits(gbits)) and torch.equal(_bits(d2), _bits(delta)) and torch.equal(_bits(db), _bits(dbias))):
            fails.append("%s form: d(qkv), delta or dbias differ in bits from the one-call form" % form)
        err = ((db.double() - bref).abs() / ball).nan_to_num(nan=INF)
        if float(err.max()) > 1:
            i = int(err.argmax())
            fails.append("dbias (%s form) column %d: got %.9g, column sum %.9g, allowed %.3g" % (form, i, float(db[i]), float(bref[i]), float(ball[i])))
    # delta_ready with a delta worked out here, and with that delta + 1: see _run
    own = (dout.double() * res["out"].double()).view(B * T, nH, DH).sum(-1).float()
    _, res["dqkv_own"], d4, _ = bwd(False, delta=own)
    if not torch.equal(_bits(d4), _bits(own)):
        fails.append("delta_ready: the delta handed in was overwritten")
    _, g5, _, _ = bwd(False, delta=own + 1.0)
    if bool((keep != 0).any()) and (torch.equal(g5[..., :D], res["dqkv_own"][..., :D]) or torch.equal(g5[..., D:2 * D], res["dqkv_own"][..., D:2 * D])):
        fails.append("delta_ready: dQ or dK do not move with the delta handed in -- the call computed its own")
    return res, fails


def _run(fam, qkv, dout, keep, nH, drop_p=0.0, seed=0, forms=True):
    """forward + backward of one case through framed buffers.  Returns the CPU results and a list of failures of the checks that
    need no reference: writes outside a buffer, the three forms of the bias gradient, delta_ready, repeatability."""
    if fam == "x3":
        return _run_x3(qkv, dout, keep, nH, drop_p, seed, forms)
    f = FAM[fam]
    dtype = f["dtype"]
    B, T, D3 = qkv.shape
    D = D3 // 3
    fails = []
    # inputs: NaN around qkv and dout, a nonzero value around keep -- a read past row T that matters shows up in the results
    fq = _Framed((B, T, 3 * D), dtype, 0, NAN, qkv)
    fd = _Framed((B, T, D), dtype, 0, NAN, dout)
    fk = _Framed((B, T), torch.int32, 0, 7, keep)
    fo = _Framed((B, T, D), dtype, NAN, SENT)
    fl = _Framed((B, nH, T), F32, NAN, SENT)
    kw = dict(drop_p=drop_p, drop_seed=seed)
    hip.attn_fwd(fq.t, fk.t, fo.t, fl.t, B, T, nH, DH, **kw)
    code = hip.dt(fq.t)
    nrows = hip.attn_bwd_bias_rows(B, T, code)

    def bwd(dbias_form, delta=None):
        fg = _Framed((B, T, 3 * D), dtype, NAN, SENT)
        fdel = _Framed((B * T, nH), F32, NAN, SENT, delta)
        fdq = _Framed((B * T, D), F32, NAN, SENT)
        fws = _Framed((nrows, 3 * D), F32, NAN, SENT)
        dbias = torch.full((3 * D,), 0.5, device=DEV)
        flags, ws = 0, fws.t
        if dbias_form == "atomics":
            ws = None
        elif dbias_form == "deferred":
            flags = hip.ATTN_DBIAS_ROWS
        hip.attn_bwd(fq.t, fk.t, fo.t, fd.t, fl.t, fdel.t, fdq.t, fg.t, B, T, nH, DH, delta_ready=delta is not None,
                     dbias=dbias, dbias_ws=ws, flags=flags, **kw)
        if dbias_form == "deferred":
            if not torch.equal(dbias, torch.full_like(dbias, 0.5)):
                fails.append("deferred dbias: the call itself summed something")
            hip.colsum_batch([(fws.t.data_ptr(), dbias.data_ptr(), 3 * D, hip.attn_bwd_dbias_rows(code, B, T), 3 * D)])
        for nm, fr in (("dqkv", fg), ("delta", fdel), ("dq32", fdq), ("dbias_ws", fws)):
            if not fr.untouched():
                fails.append("%s (%s form): written outside the buffer" % (nm, dbias_form))
        return fg.t.cpu(), fdel.t.cpu(), dbias.cpu()

    dqkv, delta, dbias = bwd("rows")
    for nm, fr in (("qkv", fq), ("dout", fd), ("keep", fk), ("out", fo), ("lse", fl)):
        if not fr.untouched():
            fails.append("%s: written outside the buffer" % nm)
    out, lse = fo.t.cpu(), fl.t.cpu()
    res = dict(out=out, lse=lse, dqkv=dqkv, delta=delta)
    if bool(delta.isnan().any()):
        fails.append("delta: %d elements NaN or never written" % int(delta.isnan().sum()))
    if not forms:
        return res, fails
    # the fused bias gradient: 0.5 + column sums of d(qkv) AS STORED; an fp32 sum of n = B T terms in any order is within
    # n 2^-24 of the sum of their magnitudes
    g64 = dqkv.double().view(B * T, 3 * D)
    bref, ball = 0.5 + g64.sum(0), B * T * 2.0 ** -24 * (0.5 + g64.abs().sum(0)) + 1e-30
    # Two calls give the same bits, except (a) the tiled dQ with more than one key block: its blocks add into dq32 with fp32
    # atomics, whose order is the hardware's; (b) the atomics form of dbias, for the same reason.
    nkb = 1 if f["whole"] else -(-T // (128 if dtype == F32 else 256))
    forms_ = [("rows", dbias), ("atomics", None)] + ([("deferred", None)] if hip.attn_bwd_dbias_rows(code, B, T) > 0 else [])
    for form, db in forms_:
        if db is None:
            g2, d2, db = bwd(form)
            same = torch.equal(_bits(g2[..., D:]), _bits(dqkv[..., D:])) and torch.equal(_bits(d2), _bits(delta))
            if nkb == 1:
                same = same and torch.equal(_bits(g2), _bits(dqkv))
            if not same:
                fails.append("d(qkv) of the %s form differs in bits from the partial-rows form" % form)
            if form == "deferred" and not torch.equal(_bits(db), _bits(dbias)):
                fails.append("deferred dbias differs in bits from the partial-rows form")
        err = ((db.double() - bref).abs() / ball).nan_to_num(nan=INF)
        if float(err.max()) > 1:
            i = int(err.argmax())
            fails.append("dbias (%s form) column %d: got %.9g, column sum %.9g, allowed %.3g" % (form, i, float(db[i]), float(bref[i]), float(ball[i])))
    # delta_ready: the delta of the first call handed back in.  Whole-head: the same bits; tiled with several key blocks: dQ
    # within twice the atomics' order error, i.e. inside the reference bound that the caller applies to the first result
    g3, _, _ = bwd("rows", delta=delta)
    if not torch.equal(_bits(g3[..., D:]), _bits(dqkv[..., D:])) or (nkb == 1 and not torch.equal(_bits(g3), _bits(dqkv))):
        fails.append("delta_ready: d(qkv) differs in bits from the call that computed delta itself")
    res["dqkv_ready"] = g3
    # That alone cannot tell a call that uses the delta it is handed from one that computes its own.  So a third call gets a delta
    # worked out here, sum_d dO_d out_d of the stored out in float64, rounded to fp32 (the caller holds its result to the reference
    # bounds, whose e_delta covers it), and a fourth the same delta + 1: dS = p (dP - delta) falls by p, so dQ and dK move
    own = (dout.double() * out.double()).view(B * T, nH, DH).sum(-1).float()
    res["dqkv_own"], d4, _ = bwd("rows", delta=own)
    if not torch.equal(_bits(d4), _bits(own)):
        fails.append("delta_ready: the delta handed in was overwritten")
    g5, _, _ = bwd("rows", delta=own + 1.0)
    if bool((keep != 0).any()) and (torch.equal(_bits(g5[..., :D]), _bits(res["dqkv_own"][..., :D])) or torch.equal(_bits(g5[..., D:2 * D]), _bits(res["dqkv_own"][..., D:2 * D]))):
        fails.append("delta_ready: dQ or dK do not move with the delta handed in -- the call computed its own")
    return res, fails


def _heads(res, nH):
    """the kernels' outputs in the reference's layout"""
    B, T, D = res["out"].shape
    h = lambda x: x.view(B, T, nH, DH).transpose(1, 2)
    g = res["dqkv"]
    return dict(out=h(res["out"]), lse=res["lse"], dQ=h(g[..., :D]), dK=h(g[..., D:2 * D]), dV=h(g[..., 2 * D:]))


def _check_delta(name, r, a, res, fails):
    """the delta the backward left behind: sum_d dO_d out_d of the STORED out, a 64-term fp32 sum"""
    B, nH, T = r["has"].shape
    o = res["out"].double().view(B, T, nH, DH).transpose(1, 2)
    ref = (r["dO"] * o).sum(-1)
    al = 2.0 ** -18 * (r["dO"] * o).abs().sum(-1) + 1e-30
    got = res["delta"].double().view(B, T, nH).transpose(1, 2)
    bad = ~((got - ref).abs() <= al)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        fails.append("%s delta: %d outside the bound, first at %s: got %.9g, ref %.9g, allowed %.3g" % (name, int(bad.sum()), i, float(got[i]), float(ref[i]), float(al[i])))


def _kernel_cases(fam, cases, worst):
    """run the cases on the device and judge them; returns the failures"""
    allf = []
    for cs in cases:
        qkv, dout, keep = _case(fam, *cs)
        nH = cs[0][1]
        name = _name(fam, *cs)
        res, fails = _run(fam, qkv, dout, keep, nH)
        r, a = _ref_of(fam, *cs)
        w, f2 = _judge(name, r, a, _heads(res, nH))
        _check_delta(name, r, a, res, f2)
        if "dqkv_ready" in res:
            _, f3 = _judge(name + " delta_ready", r, a, _heads(dict(res, dqkv=res["dqkv_ready"]), nH), ["dQ", "dK", "dV"])
            f2 += f3
        if "dqkv_own" in res:          # delta_ready with the test's own delta of the stored out: the reference bounds (e_delta covers it)
            _, f3 = _judge(name + " delta_ready (own delta)", r, a, _heads(dict(res, dqkv=res["dqkv_own"]), nH), ["dQ", "dK", "dV"])
            f2 += f3
        for qn in QUANT:
            worst[qn] = max(worst.get(qn, 0.0), w[qn])
        allf += [name + ": " + x for x in fails] + f2
    return allf


def _kernel_params():
    out = []
    for fam in FAM:
        for T in FAM[fam]["Ts"]:
            out.append(pytest.param(fam, BASE, T, "masks", id="%s-T%d-masks" % (fam, T)))
            if T in FAM[fam]["sub"]:
                out.append(pytest.param(fam, BASE, T, "values", id="%s-T%d-values" % (fam, T)))
    return out + [pytest.param(fam, g, T, "masks", id="%s-B%d-nH%d-T%d-masks" % (fam, g[0], g[1], T)) for fam, g, T in EXTRA_GEOM]


@gpu
@pytest.mark.parametrize("fam,geom,T,group", _kernel_params())
def test_attention_against_float64(fam, geom, T, group):
    """section 4: every mask pattern with randn values ("masks"), and at the T subset of the family every value pattern on four
    masks ("values")"""
    if group == "masks":
        cases = [(geom, T, mk, "randn") for mk in MASKS]
    else:
        cases = [(geom, T, mk, vl) for vl in VALUES for mk in VALUE_MASKS]
    cases = [cs for cs in cases if _case(fam, *cs) is not None]
    worst = {}
    fails = _kernel_cases(fam, cases, worst)
    print("%s B=%d nH=%d T=%d: %d cases, worst err / allowed %s" % (fam, geom[0], geom[1], T, len(cases), {k: round(v, 3) for k, v in worst.items()}))
    assert not fails, "%d failures, first 12:\n" % len(fails) + "\n".join(fails[:12])


# =====================================================================================================================
# 5. metamorphic checks of the whole-head path (no dropout): bit for bit
# =====================================================================================================================
def _plain(qkv, dout, keep, nH):
    """out, lse, d(qkv) on the CPU, through plain buffers"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    qd, dd, kd = qkv.to(DEV), dout.to(DEV), keep.to(DEV)
    out = torch.empty(B, T, D, device=DEV, dtype=qkv.dtype)
    lse = torch.empty(B, nH, T, device=DEV)
    hip.attn_fwd(qd, kd, out, lse, B, T, nH, DH)
    dqkv = torch.full((B, T, 3 * D), NAN, device=DEV, dtype=qkv.dtype)
    ws = torch.empty(hip.attn_bwd_bias_rows(B, T, hip.dt(qd)), 3 * D, device=DEV)
    dbias = torch.zeros(3 * D, device=DEV)
    hip.attn_bwd(qd, kd, out, dd, lse, torch.empty(B * T, nH, device=DEV), torch.empty(B * T, D, device=DEV), dqkv, B, T, nH, DH,
                 dbias=dbias, dbias_ws=ws)
    return out.cpu(), lse.cpu(), dqkv.cpu(), dbias.cpu()


@gpu
@pytest.mark.parametrize("T", [33, 236, 385])
@pytest.mark.parametrize("mask", ["holes", "lpad17"])
def test_whole_head_metamorphic(T, mask):
    fam = "wh256" if T <= 256 else "wh512"
    B, nH = BASE
    D = nH * DH
    qkv, dout, keep = _case(fam, BASE, T, mask, "randn")
    o1, l1, g1, b1 = _plain(qkv, dout, keep, nH)
    # two identical calls
    o2, l2, g2, b2 = _plain(qkv, dout, keep, nH)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in ((o1, o2), (l1, l2), (g1, g2), (b1, b2))), "two identical calls differ"
    # other k and v at the padded positions: a padded key is invisible to every query, so nothing changes anywhere (but the sign of
    # the zeros that are the padded keys' own dK / dV)
    pad = keep == 0
    kp = ~pad
    q2 = qkv.clone()
    q2[..., D:][pad] = (qkv[..., D:][pad].float() * -3.0 + 1.0).to(BF)
    o3, l3, g3, b3 = _plain(q2, dout, keep, nH)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in ((o1, o3), (l1, l3), (g1[kp], g3[kp]), (g1[pad][:, :D], g3[pad][:, :D]), (b1, b3))), "a padded key's k or v reaches a result"
    assert bool((g3[pad][:, D:] == 0).all()), "dK / dV of a padded key"
    # other q and dout there as well: a padded position is still a live QUERY, so its own out, lse and dQ change, and so do dK / dV
    # of the kept keys it sees; out, lse and dQ of every kept position keep their bits, dK / dV of the padded keys stay 0
    d2 = dout.clone()
    q2[..., :D][pad] = (qkv[..., :D][pad].float() * 2.0 - 1.0).to(BF)
    d2[pad] = (d2[pad].float() * 5.0 - 2.0).to(BF)
    o3, l3, g3, _ = _plain(q2, d2, keep, nH)
    assert torch.equal(_bits(o1[kp]), _bits(o3[kp])), "out of a kept position depends on a padded one"
    assert torch.equal(_bits(l1.transpose(1, 2)[kp]), _bits(l3.transpose(1, 2)[kp])), "lse of a kept position depends on a padded one"
    assert torch.equal(_bits(g1[kp][:, :D]), _bits(g3[kp][:, :D])), "dQ of a kept position depends on a padded one"
    assert bool((g3[pad][:, D:] == 0).all()), "dK / dV of a padded key"
    # other values behind position t: out and lse up to t keep their bits
    t = T // 2
    q4 = qkv.clone()
    q4[:, t + 1:] = (q4[:, t + 1:].float() * 2.0 - 1.0).to(BF)
    o4, l4, _, _ = _plain(q4, dout, keep, nH)
    assert torch.equal(_bits(o1[:, :t + 1]), _bits(o4[:, :t + 1])) and torch.equal(_bits(l1[..., :t + 1]), _bits(l4[..., :t + 1])), "out / lse depend on a later position"
    # a batch row alone
    for b in range(B):
        o5, l5, g5, _ = _plain(qkv[b:b + 1], dout[b:b + 1], keep[b:b + 1], nH)
        assert torch.equal(_bits(o5[0]), _bits(o1[b])) and torch.equal(_bits(l5[0]), _bits(l1[b])) and torch.equal(_bits(g5[0]), _bits(g1[b])), "batch row %d alone differs" % b


# =====================================================================================================================
# 6. dropout
# =====================================================================================================================
DROP_CASES = [("wh256", 64), ("wh256", 200), ("wh256", 256), ("wh512", 320), ("wh512", 512), ("tiled16", 513), ("tiled32", 129), ("tiled32", 257), ("x3", 129)]
DROP_P = [0.1, 0.3]


def _drop_prob(fam, p):
    """(keep probability, scale) of the family: the whole-head kernels keep with probability keepq / 4096, keepq = 4096 -
    round(p 4096), and scale by 4096 / keepq; the others keep where a 32-bit hash >= thresh = floor(p 2^32), scale 2^32 / (2^32 - thresh)"""
    if FAM[fam]["whole"]:
        keepq = 4096 - ((hip.drop_thresh(p) + 0x80000) >> 20)
        return keepq / 4096.0, 4096.0 / keepq
    th = hip.drop_thresh(p)
    return 1.0 - th / 2.0 ** 32, 2.0 ** 32 / (2.0 ** 32 - th)


def _causal_count(T):
    return T * (T + 1) // 2


def test_kept_fraction_interval_against_the_neighbouring_levels():
    """the assertion of section 6 on the kept fraction, worked out without a GPU: 5 binomial standard deviations over the
    T (T + 1) / 2 causal elements of one matrix against the distance to the nearest plausible wrong keep probability, 1 - p +- 2^-6.
    The interval is narrower than that distance from T = 256 on, and at T = 200 for p = 0.1; at T = 64 and 129 (and T = 200,
    p = 0.3) it is wider, so there the kernel test's assertion still holds the fraction to the family's probability but could not
    tell it from the neighbouring level -- the larger T of the same kernel family do that."""
    wide = set()
    for fam, T in DROP_CASES:
        for p in DROP_P:
            pk, scale = _drop_prob(fam, p)
            assert abs(pk - (1 - p)) <= 2.0 ** -13 + 1e-12 and abs(pk * scale - 1.0) < 1e-12, (fam, p, pk)
            half = 5.0 * math.sqrt(pk * (1 - pk) / _causal_count(T))
            if not half < 2.0 ** -6 - abs(pk - (1 - p)):
                wide.add((T, p))
    assert wide == {(64, 0.1), (64, 0.3), (129, 0.1), (129, 0.3), (200, 0.3)}, sorted(wide)


def _recover_masks(fam, B, nH, T, p, seed):
    """the keep matrix of every (b, h): q = k = 0 makes attention uniform, V = unit vectors over 64 keys at a time, so
    out[t, j] != 0 iff element (t, c0 + j) was kept (the probe of test_attention_dropout_consistency)"""
    dtype = FAM[fam]["dtype"]
    D = nH * DH
    keep = torch.ones(B, T, dtype=torch.int32, device=DEV)
    out = torch.empty(B, T, D, device=DEV, dtype=dtype)
    lse = torch.empty(B, nH, T, device=DEV)
    M = torch.zeros(B, nH, T, T)
    for c0 in range(0, T, DH):
        n = min(DH, T - c0)
        probe = torch.zeros(B, T, 3 * D, dtype=dtype)
        for h in range(nH):
            probe[:, c0:c0 + n, 2 * D + h * DH:2 * D + h * DH + n] = torch.eye(n).to(dtype)
        if fam == "x3":
            out = out.view(B * T, D)
            hip.attn_fwd_x3(hip.split_planes(probe.view(B * T, 3 * D).to(DEV), B * T, 3 * D, hip.Planes.empty(B * T, 3 * D, DEV)), keep, out, None, lse,
                            B, T, nH, DH, drop_p=p, drop_seed=seed)
        else:
            hip.attn_fwd(probe.to(DEV), keep, out, lse, B, T, nH, DH, drop_p=p, drop_seed=seed)
        M[:, :, :, c0:c0 + n] = (out.float().cpu().view(B, T, nH, DH).transpose(1, 2)[..., :n] != 0).float()
    return M


@gpu
@pytest.mark.parametrize("p", DROP_P)
@pytest.mark.parametrize("fam,T", DROP_CASES)
def test_attention_dropout_against_float64(fam, T, p):
    B, nH = BASE
    seed = 11 + T
    pk, scale = _drop_prob(fam, p)
    M = _recover_masks(fam, B, nH, T, p, seed)
    tri = torch.tril(torch.ones(T, T))
    # independence: the six matrices pairwise different, and another seed gives other matrices
    flat = (M * tri).view(B * nH, -1)
    for i in range(B * nH):
        for j in range(i):
            assert not torch.equal(flat[i], flat[j]), "heads %d and %d share a dropout mask" % (j, i)
    M2 = _recover_masks(fam, B, nH, T, p, seed + 1)
    assert all(not torch.equal((M2 * tri).view(B * nH, -1)[i], flat[i]) for i in range(B * nH)), "the mask ignores the seed"
    # kept fraction of each matrix over the causal elements: within 5 binomial standard deviations of the family's probability
    half = 5.0 * math.sqrt(pk * (1 - pk) / _causal_count(T))
    frac = flat.sum(1) / tri.sum()
    assert bool(((frac - pk).abs() <= half).all()), (frac.tolist(), pk, half)
    # forward and backward against the reference that uses the recovered matrices
    qkv, dout, keep = _case(fam, BASE, T, "holes", "randn")
    res, fails = _run(fam, qkv, dout, keep, nH, drop_p=p, seed=seed, forms=False)
    r = _reference(qkv, dout, keep, nH, M.double() * scale)
    name = _name(fam, BASE, T, "holes", "randn") + " p=%g" % p
    w, f2 = _judge(name, r, _bounds(r, fam), _heads(res, nH))
    print(name, "worst err / allowed", {k: round(v, 3) for k, v in w.items()})
    assert not fails + f2, "\n".join((fails + f2)[:12])


# =====================================================================================================================
# 7. the kernels behind the environment switches, each in a child process
# =====================================================================================================================
ENV_SETTINGS = {
    "kv2-0": {"MMTG_ATTN_KV2": "0"},
    "kv-nw4": {"MMTG_ATTN_KV2": "0", "MMTG_ATTN_KV_NW": "4"},
    "kv-nw8": {"MMTG_ATTN_KV2": "0", "MMTG_ATTN_KV_NW": "8"},          # T <= 256: the full-wave build; T > 256: the half-wave one
    "kv-nw16": {"MMTG_ATTN_KV2": "0", "MMTG_ATTN_KV_NW": "16"},
    "tiled": {"MMTG_ATTN_TILED": "1"},
}
# The library does not report which kernel a call took, so the names above are pinned by hand to the getenv calls of
# mmtg_attn_bwd / attn_route_tiled in csrc/attention.hip: a renamed switch would turn a child into a rerun of the default
# path.  For MMTG_ATTN_TILED the parent can tell: the tiled kernels draw their dropout masks from another hash than the whole-head
# ones, so the child's dropout output must differ in bits from the parent's own (_drop_digest).  The 16-key dK / dV builds behind
# KV2 / KV_NW are written to give the bits of the default build, so nothing the entries return tells them apart.
CHILD_T = [17, 33, 65, 129, 236, 256, 257, 385, 512]
# a run of the child takes 7 to 12 s of wall time for every setting (import, 9 T x up to 14 cases, two dropout cases); the limit
# is generous because a shared machine may be slow, and it is there only to end a hang
CHILD_LIMIT = 120


def _drop_digest(out):
    return hashlib.sha1(out.contiguous().view(torch.int16).numpy().tobytes()).hexdigest()


def _child_main(out_path):
    """the bf16 subset through the same reference and bounds: one T per edge, every mask with randn, loud padding, two dropout cases (T = 200 and 320)"""
    tiled = "MMTG_ATTN_TILED" in os.environ
    report = {"worst": {}, "fails": [], "cases": 0}
    for T in CHILD_T:
        fam = "tiled16" if tiled else ("wh256" if T <= 256 else "wh512")
        cases = [(BASE, T, mk, "randn") for mk in MASKS] + [(BASE, T, mk, "loud") for mk in VALUE_MASKS]
        cases = [cs for cs in cases if _case(fam, *cs) is not None]
        report["fails"] += _kernel_cases(fam, cases, report["worst"])
        report["cases"] += len(cases)
    for T in (200, 320):
        fam = "tiled16" if tiled else ("wh256" if T <= 256 else "wh512")
        B, nH = BASE
        _, scale = _drop_prob(fam, 0.3)
        M = _recover_masks(fam, B, nH, T, 0.3, 5)
        qkv, dout, keep = _case(fam, BASE, T, "holes", "randn")
        res, fails = _run(fam, qkv, dout, keep, nH, drop_p=0.3, seed=5, forms=False)
        r = _reference(qkv, dout, keep, nH, M.double() * scale)
        w, f2 = _judge(_name(fam, BASE, T, "holes", "randn") + " p=0.3", r, _bounds(r, fam), _heads(res, nH))
        report["fails"] += fails + f2
        report["worst"]["dropout"] = max(report["worst"].get("dropout", 0.0), max(w.values()))
        report["cases"] += 1
        if T == 200:
            report["drop_digest"] = _drop_digest(res["out"])
    with open(out_path, "w") as fh:
        json.dump(report, fh)


@gpu
@pytest.mark.parametrize("setting", list(ENV_SETTINGS))
def test_attention_variants_in_a_child_process(setting, tmp_path):
    """the switches are read once per process, so each setting gets a fresh child (started, never exec'd into; never retried).  A
    child that ends by a signal or at its time limit ends the whole session: nothing more may start on a GPU that has faulted"""
    env = dict(os.environ, **ENV_SETTINGS[setting])
    out = str(tmp_path / "report.json")
    try:
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        pytest.exit("attention child process (%s) ran into its time limit of %d s: treated as a hang, nothing more is started" % (setting, CHILD_LIMIT), returncode=3)
    if pr.returncode < 0:
        pytest.exit("attention child process (%s) ended by signal %d:\n%s" % (setting, -pr.returncode, pr.stderr[-2000:]), returncode=3)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    with open(out) as fh:
        report = json.load(fh)
    print("%s: %d cases, worst err / allowed %s" % (setting, report["cases"], {k: round(v, 3) for k, v in report["worst"].items()}))
    assert not report["fails"], "%d failures, first 12:\n" % len(report["fails"]) + "\n".join(report["fails"][:12])
    if setting == "tiled" and "MMTG_ATTN_TILED" not in os.environ:
        # the same dropout case on this process's default route, the whole-head kernels
        qkv, dout, keep = _case("wh256", BASE, 200, "holes", "randn")
        res, _ = _run("wh256", qkv, dout, keep, BASE[1], drop_p=0.3, seed=5, forms=False)
        assert report["drop_digest"] != _drop_digest(res["out"]), "MMTG_ATTN_TILED=1 did not reach the tiled kernels: the child's dropout output is the whole-head one"
    assert report["cases"] >= 100 and all(v <= 1.0 for v in report["worst"].values()), report["worst"]


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "child", "usage: test_attn_ops_gpu.py child <report.json>"
    _child_main(sys.argv[2])
