"""The training step's tail, one kernel at a time, against float64 restatements (csrc/loss.hip, csrc/optim.hip).

tests/test_ops_gpu.py holds one or two cases per kernel at one shape against fp32 references; the full-model golden tests notice
a wrong loss or update late and cannot say which kernel, or which branch of it, went wrong.  Here every case hands ONE entry
inputs already rounded to its storage type and compares what it wrote with the same operation restated in float64 on the CPU:

  1. row log-sum-exp and nll (mmtg_loss_fwd) at every row length where row_lse_kernel changes path: scalar tail only, one slice,
     a second slice for thread 0 only, the last all-in-registers row, the first streaming row, GPT-2's vocabulary;
  2. the per-sample loss (sample_loss_kernel) over both trips of its 16-wave sample loop and 1 .. 129+ terms of its lane loop,
     with samples steered to p -> 1, p ~ 0.3 and an overflowing exp;
  3. d(logits) (mmtg_loss_bwd in its four storage forms, mmtg_loss_bwd_x3) with lm_coef, P = 0, scalar shapes, ldd > Vpad;
  4. the gradient norm (mmtg_sumsq), exact on integer data across the tail / 256-partial / 2048-workgroup / second-trip edges;
  5. AdamW (mmtg_adamw): p, m and v of three state-carrying steps, every element, with wd, clip, count, the scalar fallback of a
     misaligned pointer and the bf16 plane copies;
  6. slab sums, casts, axpy and the padded row cast, exact.

Every bound is derived where it is defined; the two that rest on a measurement (the fp32 yardsticks of sections 1 and 2) are
recorded in docs/experiments.md, "Loss and optimizer kernels against float64".  The tests without the gpu mark run the float32
CPU restatements of the same operations through the same bounds on the same inputs: a bound the restatement cannot meet is a
wrong derivation, not a kernel bug.
"""
import functools
import math

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from oracle import mmtg_oracle as O
from helpers import rnd, tol

gpu = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32
SENT = 1234.0                # sentinel of columns / elements a kernel must leave alone (exact in bf16)


def _bits(t):
    """the tensor's storage as integers: NaN compares equal to the same NaN, -0 differs from +0"""
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _ulp32(x):
    """spacing of fp32 at |x| (x float64) as float64"""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _within(name, got, ref, allow):
    """every element of got within allow of ref (NaN anywhere fails)"""
    err = (got.double() - ref).abs()
    ok = err <= allow
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d/%d outside the bound, first at %s: got %.9g, ref %.9g, allowed %.3g; worst err/allowed %.3g" % (
            name, len(bad), ok.numel(), i, float(got[i]), float(ref[i]), float(allow[i]) if allow.dim() else float(allow),
            float((err / allow.clamp(min=1e-300)).nan_to_num(nan=float("inf")).max())))


# =====================================================================================================================
# 1. row log-sum-exp and nll
# =====================================================================================================================
LSE_V = [1, 7, 8, 333, 2048, 2049, 2055, 16384, 16391, 16392, 18437, 50257]
LB, LP, LL = 2, 1, 3
LT = LP + LL
LM = LB * LT                  # 8 rows per call
# The fp32 yardstick: the worst error of CPU torch.logsumexp in float32 against float64 on these rows, as a fraction of
# max(1, |lse|) (an lse is max + log(sum): its error is the sum's relative error plus roundings at the magnitude of the
# result), on the rows as stored in fp32 (False) and in bf16 (True).  Measured by test_lse_yardstick_float32_cpu below, recorded
# in docs/experiments.md; the kernel gets 4 times it.
LSE_YARD = {False: 5.7e-8, True: 7.6e-8}
LSE_FACTOR = 4


def _probe_cols(V):
    """where a probe row holds its single 0: the ends of the first slices, the last slice and the scalar tail (V8 = V & ~7), the
    last register slice (16383), the first column only the streaming loop reads (16384), and the first columns of the second
    streaming trip of threads 0, 1 and 255 (2048, 2056, 4088)"""
    V8 = V & ~7
    return sorted({c for c in (0, 7, 8, 2047, 2048, 2056, 4088, V8 - 1, V8, V - 1, 16383, 16384) if 0 <= c < V})


@functools.lru_cache(maxsize=None)
def _lse_rows(V, bf):
    """[calls, 8, V] in the storage type: probe rows, an ascending and a descending ramp over 40, a random row at +80 and the same
    at -80, a constant row; random rows fill the last call"""
    rows = []
    for c in _probe_cols(V):
        r = torch.full((V,), -30.0)
        r[c] = 0.0
        rows.append(r)
    ramp = torch.linspace(-20.0, 20.0, V) if V > 1 else torch.zeros(1)
    r = rnd(V, seed=V)
    rows += [ramp, ramp.flip(0), 2 * r + 80, 2 * r - 80, torch.full((V,), 3.25)]
    k = 0
    while len(rows) % LM:
        k += 1
        rows.append(rnd(V, seed=V + k, scale=2.0))
    return torch.stack(rows).to(BF if bf else F32).view(-1, LM, V)


def _lse_ref(x):
    """float64 log-sum-exp over the last axis of the stored values"""
    x = x.double()
    m = x.max(-1, keepdim=True).values
    return (m + (x - m).exp().sum(-1, keepdim=True).log()).squeeze(-1)


def _lse_allow(x, ref, bf):
    """fp32 logits: LSE_FACTOR times the yardstick, not less than 2 ulp of the fp32 result (the stored lse is itself rounded).
    bf16 logits go through the hardware exponential of x * log2(e): the product x * log2(e) is rounded at the magnitude of
    |x - max| (one ulp of the argument moves the exponential by |x - max| 2^-23 relative) and the instruction is good to about an
    ulp more; weighted by the softmax that is sum_v softmax_v (|x_v - max| + 2) 2^-23 of the sum, hence of the lse."""
    a = torch.maximum(LSE_FACTOR * LSE_YARD[bool(bf)] * ref.abs().clamp(min=1.0), 2 * _ulp32(ref))
    if bf:
        xd = x.double()
        m = xd.max(-1, keepdim=True).values
        sm = (xd - ref.unsqueeze(-1)).exp()
        a = a + (sm * ((xd - m).abs() + 2)).sum(-1) * 2.0 ** -23
    return a


def _lse_labels(V, k):
    """[B, T] label table cat(topic_ids, targets) of call k: the labels of rows 0 .. T-2 are columns 1 .. T-1; they sit at 0,
    V8 - 1, V8 and V - 1 (rotated by the call) and at two random columns"""
    V8 = V & ~7
    edge = [c for c in dict.fromkeys((0, V8 - 1, V8, V - 1)) if 0 <= c < V]
    g = torch.Generator().manual_seed(7 * V + k)
    lab = torch.randint(0, V, (LB, LT), generator=g)
    flat = [edge[(i + k) % len(edge)] for i in range(4)]
    lab[0, 1:] = torch.tensor(flat[:3])
    lab[1, 1] = flat[3]
    return lab


def _loss_fwd(x, V, lab, ratings, stage, label_zero, B, P, L, den):
    """x: [B * (P + L), V] in its storage type -> (nll, lse, sample_ce, coef, scalars) as float64 on the CPU.  The rows are padded
    to the next multiple of 8 plus 8 columns of NaN (the header: columns >= V are ignored); every output starts as NaN"""
    M = x.shape[0]
    ldl = (V + 7) // 8 * 8 + 8
    buf = torch.full((M, ldl), NAN, dtype=x.dtype)
    buf[:, :V] = x
    outs = [torch.full((n,), NAN, device=DEV) for n in (M, M, B, B, 2)]
    topic = lab[:, :P].contiguous().to(DEV) if P else None          # (no topic table at P = 0)
    hip.loss_fwd(buf.to(DEV), ldl, V, topic, lab[:, P:].contiguous().to(DEV), None if ratings is None else ratings.to(DEV),
                 stage, label_zero, B, P, L, den, *outs)
    return [o.cpu().double() for o in outs]


def _check_rows(name, x, V, lab, lse, nll, bf, B, T):
    """lse of every row, nll of every row (exactly 0 on each sample's last)"""
    ref = _lse_ref(x)
    allow = _lse_allow(x, ref, bf)
    _within(name + " lse", lse, ref, allow)
    xl = x.double().view(B, T, V)[:, :-1].gather(-1, lab[:, 1:, None]).squeeze(-1)
    nref = ref.view(B, T)[:, :-1] - xl
    # nll = lse - logit[label] in fp32: the lse allowance, plus the ulp of the label's logit for the rounded difference
    _within(name + " nll", nll.view(B, T)[:, :-1], nref, allow.view(B, T)[:, :-1] + _ulp32(xl))
    assert bool((nll.view(B, T)[:, -1] == 0).all()), name + ": nll of a sample's last row must be exactly 0"


@gpu
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", LSE_V)
def test_row_lse_and_nll(V, bf):
    rows = _lse_rows(V, bf)
    for k in range(rows.shape[0]):
        x = rows[k]
        lab = _lse_labels(V, k)
        nll, lse, _, _, _ = _loss_fwd(x, V, lab, None, 1, False, LB, LP, LL, float(LB))
        _check_rows("V=%d call %d" % (V, k), x, V, lab, lse, nll, bf, LB, LT)
    x = rows[0]
    # label_zero: every label is column 0, whatever the tables hold
    lab = _lse_labels(V, 0)
    nll, lse, _, _, _ = _loss_fwd(x, V, lab, None, 1, True, LB, LP, LL, float(LB))
    _check_rows("V=%d label_zero" % V, x, V, torch.zeros_like(lab), lse, nll, bf, LB, LT)
    # out-of-range labels clamp into the row: -3 reads column 0, V + 5 reads column V - 1 (include/mmtg_hip.h)
    lab = _lse_labels(V, 0)
    lab[0, 2], lab[1, 3] = -3, V + 5
    nll, lse, _, _, _ = _loss_fwd(x, V, lab, None, 1, False, LB, LP, LL, float(LB))
    _check_rows("V=%d clamped labels" % V, x, V, lab.clamp(0, V - 1), lse, nll, bf, LB, LT)


def test_lse_yardstick_float32_cpu():
    """the yardstick itself: CPU torch.logsumexp in float32 against float64 on every row of section 1.  LSE_YARD holds the figures
    this test printed where they were measured (docs/experiments.md); torch's summation order depends on the CPU it runs on, so
    what is asserted is that it stays inside the kernel's allowance, 4 times LSE_YARD.  Also: the probe and constant rows'
    float64 values are what the row contents say they must be"""
    worst = {}
    for bf in (False, True):
        w = 0.0
        for V in LSE_V:
            x = _lse_rows(V, bf).reshape(-1, V)
            ref = _lse_ref(x)
            got = torch.logsumexp(x.float(), -1).double()
            w = max(w, float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max()))
            npb = len(_probe_cols(V))
            assert torch.allclose(ref[:npb], torch.full((npb,), math.log1p((V - 1) * math.exp(-30.0)), dtype=torch.float64), rtol=0, atol=1e-11)
            assert abs(float(ref[npb + 4]) - (3.25 + math.log(V))) < 1e-12
            assert bool(torch.isfinite(ref).all())
        worst["bf16" if bf else "f32"] = w
        assert not math.isnan(w) and w <= LSE_FACTOR * LSE_YARD[bf], worst
    print("float32 torch.logsumexp against float64, worst err / max(1, |lse|):", worst)


# =====================================================================================================================
# 2. per-sample loss
# =====================================================================================================================
SV = 40
S_B = [1, 16, 17, 33, 40]
S_PL = [(0, 2), (0, 65), (15, 50), (1, 64), (2, 64), (15, 130)]
STAGES = [1, 2, 3]
QUANT = ["sample_ce", "coef", "scalars[0]", "scalars[1]"]
# The fp32 yardstick of each quantity: the worst error of the float32 oracle (O.my_loss, O.lm_loss_shifted, the oracle's
# cross-entropy line and its autograd coefficient) against float64, in units of the project's fp32 tolerance
# atol + rtol |ref| = tol(float32).  Measured over all 90 cases by test_sample_loss_yardstick_float32_cpu, recorded in
# docs/experiments.md.  The kernel gets 4 times it, and never less than one unit.
SAMPLE_YARD = {"sample_ce": 0.0082, "coef": 271.0, "scalars[0]": 3.2, "scalars[1]": 0.0094}
SAMPLE_FACTOR = 4


def _units(got, ref):
    """|got - ref| in units of tol(float32) at ref"""
    atol, rtol = tol(F32)
    return (got.double() - ref).abs() / (atol + rtol * ref.abs())


@functools.lru_cache(maxsize=None)
def _sample_case(B, P, L, stage):
    """logits [B, T, 40] (fp32 values), labels [B, T], ratings, batch denominator.  Sample b is steered by b + stage + L mod 6:
    0 not at all (CE about 4); 1 every label +40 but the first loss row's +9 (CE about 5e-3 / ntok, 1e-4 at 50 tokens: p is
    next to 1 and 1 - p + 1e-10 decides); 2 every label +40 (p == 1 in fp32); 3 every label +9 and a wrong logit +40 on every
    32nd loss row (CE about 1); 4 a wrong logit +100 everywhere (CE about 100: exp overflows, p = 0, the loss saturates at
    -log(1e-10) and coef is 0); 5 a wrong logit +9 everywhere (CE about 10).  Ratings run through 1 .. 5."""
    T = P + L
    g = torch.Generator().manual_seed(1000 * B + 10 * T + stage)
    x = torch.randn(B, T, SV, generator=g)
    lab = torch.randint(0, SV, (B, T), generator=g)
    wrong = (lab + 1 + torch.randint(0, SV - 1, (B, T), generator=g)) % SV
    ratings = (torch.arange(B) + stage) % 5 + 1
    r = torch.arange(T - 1)
    for b in range(B):
        kind = (b + stage + L) % 6
        l1, w1 = lab[b, 1:], wrong[b, 1:]
        if kind == 1:
            x[b, r, l1] += 40.0
            x[b, P, l1[P]] -= 31.0
        elif kind == 2:
            x[b, r, l1] += 40.0
        elif kind == 3:
            x[b, r, l1] += 9.0
            rr = r[P::32]
            x[b, rr, w1[rr]] += 40.0
        elif kind == 4:
            x[b, r, w1] += 100.0
        elif kind == 5:
            x[b, r, w1] += 9.0
    den = float(B) if stage == 1 else B + 2.5
    return x, lab, ratings, den


def _nll_ref(x, lab):
    """float64 nll [B, T] of logits [B, T, V] against labels lab[b, t + 1]; 0 on the last row"""
    B, T, V = x.shape
    lse = _lse_ref(x)
    n = torch.zeros(B, T, dtype=torch.float64)
    n[:, :-1] = lse[:, :-1] - x.double()[:, :-1].gather(-1, lab[:, 1:, None]).squeeze(-1)
    return n


def _sample_ref(nll, ratings, stage, P, L, den):
    """float64 restatement of the reference's MyLoss and GPT-2's shifted CE from the rows' nll [B, T]:
    (sample_ce [B], d l_b / d CE_b [B], scalars[0], scalars[1]); coef = the derivative / ntok / den.
    1 - p is taken as -expm1(-CE): the plain difference loses it in float64 too once CE < 1e-10."""
    B, T = nll.shape
    ntok = L - 1
    ce = nll[:, P:T - 1].sum(1) / ntok
    lm = nll[:, :T - 1].sum() / (B * (T - 1))
    if ratings is None:
        z = torch.zeros(B, dtype=torch.float64)
        return ce, z, torch.zeros((), dtype=torch.float64), lm
    y = (ratings > (4 if stage == 1 else 3)).double()
    p, omp, e = torch.exp(-ce), -torch.expm1(-ce), 1e-10
    lb = -y * torch.log(p + e) - (1 - y) * torch.log(omp + e)
    cf = -p * (-y / (p + e) + (1 - y) / (omp + e))
    return ce, cf, lb.sum() / den, lm


def _sample_oracle32(x, lab, ratings, stage, P, L, den):
    """the same four from the float32 oracle: O.my_loss (a batch mean, rescaled to the batch denominator), its autograd
    gradient read back as d l_b / d CE_b at the wrong-class element of each sample where the softmax is largest, the oracle's
    cross-entropy line for sample_ce, O.lm_loss_shifted"""
    B, T, V = x.shape
    ntok = L - 1
    xr = x.float().clone().requires_grad_(True)
    targ = lab[:, P:]
    my = O.my_loss(xr, targ, ratings, stage, P)
    my.backward()
    with torch.no_grad():
        ce = torch.nn.functional.cross_entropy(x.float()[:, P:-1].reshape(-1, V), targ[:, 1:].reshape(-1), reduction="none").view(B, ntok).mean(1)
        lm = O.lm_loss_shifted(x.float(), lab)
    sm = (x.double() - _lse_ref(x).unsqueeze(-1)).exp()
    sm.scatter_add_(-1, torch.cat([lab[:, 1:], lab[:, :1]], 1)[:, :, None], -torch.ones(B, T, 1, dtype=torch.float64))
    part = sm[:, P:T - 1].reshape(B, -1)
    # (not at a label: where the label's probability rounds to 1 in fp32 its gradient is exactly 0 and carries no coefficient)
    sel = part.abs().view(B, T - 1 - P, V).scatter(-1, lab[:, P + 1:, None], 0.0).reshape(B, -1)
    idx = sel.argmax(1, keepdim=True)
    gr = xr.grad.double()[:, P:T - 1].reshape(B, -1).gather(1, idx).squeeze(1)
    cf = gr * B * ntok / part.gather(1, idx).squeeze(1)
    return ce.double(), cf, my.detach().double() * B / den, lm.double()


def _sample_cases():
    return [(B, P, L, s) for B in S_B for (P, L) in S_PL for s in STAGES]


@gpu
@pytest.mark.parametrize("PL", S_PL, ids=lambda v: "P%d-L%d" % v)
@pytest.mark.parametrize("B", S_B)
def test_sample_loss(B, PL):
    P, L = PL
    T, ntok = P + L, L - 1
    for stage in STAGES:
        x, lab, ratings, den = _sample_case(B, P, L, stage)
        nll, lse, ce, coef, sc = _loss_fwd(x.view(B * T, SV), SV, lab, ratings, stage, False, B, P, L, den)
        name = "B=%d P=%d L=%d stage %d" % (B, P, L, stage)
        _check_rows(name, x.view(B * T, SV), SV, lab, lse, nll, False, B, T)
        rce, rcf, rmy, rlm = _sample_ref(_nll_ref(x, lab), ratings, stage, P, L, den)
        for q, got, ref in (("sample_ce", ce, rce), ("coef", coef * (ntok * den), rcf), ("scalars[0]", sc[0], rmy), ("scalars[1]", sc[1], rlm)):
            u = _units(got, ref)
            lim = max(1.0, SAMPLE_FACTOR * SAMPLE_YARD[q])
            assert bool((u <= lim).all()), "%s %s: %.3g units of tol(float32), allowed %.3g (got %s, ref %s)" % (name, q, float(u.max()), lim, got, ref)
        # the saturated samples: p = 0 exactly, so is the coefficient
        sat = rce > 95
        assert bool((coef[sat] == 0).all()), name
    # no ratings: MyLoss and its coefficients are exactly 0, the LM loss and the sample CE are still computed
    x, lab, ratings, den = _sample_case(B, P, L, 2)
    nll, lse, ce, coef, sc = _loss_fwd(x.view(B * T, SV), SV, lab, None, 2, False, B, P, L, den)
    rce, _, _, rlm = _sample_ref(_nll_ref(x, lab), None, 2, P, L, den)
    assert float(sc[0]) == 0.0 and bool((coef == 0).all())
    assert bool((_units(ce, rce) <= max(1.0, SAMPLE_FACTOR * SAMPLE_YARD["sample_ce"])).all())
    assert float(_units(sc[1], rlm)) <= max(1.0, SAMPLE_FACTOR * SAMPLE_YARD["scalars[1]"])


def test_sample_loss_yardstick_float32_cpu():
    """the float32 oracle stays within the kernel's allowance (4 times the figures of SAMPLE_YARD, which were measured with this
    test and are recorded in docs/experiments.md) of the float64 restatement on every case of section 2, and the steering reaches
    the regimes it is meant to.  One thing the oracle cannot do: where exp(CE) overflows, autograd multiplies 0 by inf and its
    coefficient is NaN (the kernel's analytic form gives the 0 of float64); those samples, and only those, are left out of the
    coefficient's figure."""
    worst = dict.fromkeys(QUANT, 0.0)
    seen = set()
    for B, P, L, stage in _sample_cases():
        x, lab, ratings, den = _sample_case(B, P, L, stage)
        ref = _sample_ref(_nll_ref(x, lab), ratings, stage, P, L, den)
        got = _sample_oracle32(x, lab, ratings, stage, P, L, den)
        ce = ref[0]
        for q, g_, r_ in zip(QUANT, got, ref):
            u = _units(g_, r_)
            if q == "coef":
                lost = torch.isnan(g_)
                assert bool((ce[lost] > 88.0).all()) and bool((r_[lost].abs() < 1e-30).all())
                u = u[~lost]
            if u.numel():
                assert not bool(torch.isnan(u).any()), (B, P, L, stage, q)
                worst[q] = max(worst[q], float(u.max()))
        seen |= {"p~1" for c in ce if 2e-6 < c < 5e-4} | {"p=1" for c in ce if c < 1e-12} | {"~1" for c in ce if 0.5 < c < 2} | {">88.8" for c in ce if c > 95}
    print("float32 oracle against float64, worst error in units of tol(float32):", worst)
    assert seen == {"p~1", "p=1", "~1", ">88.8"}, seen
    for q in QUANT:
        assert worst[q] <= max(1.0, SAMPLE_FACTOR * SAMPLE_YARD[q]), worst


# =====================================================================================================================
# 3. d(logits)
# =====================================================================================================================
BWD_SHAPES = [(333, 384, 384), (333, 384, 400), (333, 335, 335), (16392, 16392, 16392), (50257, 50264, 50264)]
BWD_FORMS = ["f32-f32", "f32-bf16", "bf16-bf16", "bf16-inplace", "x3"]
BWD_P = [0, 3]
BWD_LM = [0.0, 0.37]
BWD_GS = [1.0, 1.0 / 7.0]
BB, BL = 2, 3


def _bwd_params():
    out = []
    for shp in BWD_SHAPES:
        for form in BWD_FORMS:
            # (333, 335, 335) reads rows of stride 336: the x3 entry requires multiples of 8, and in place needs ldl == ldd
            if shp[1] % 8 and form in ("x3", "bf16-inplace"):
                continue
            for P in BWD_P:
                out.append(pytest.param(shp, form, P, id="V%d-Vpad%d-ldd%d-%s-P%d" % (shp + (form, P))))
    return out


@functools.lru_cache(maxsize=None)
def _bwd_case(V, P, bf):
    """logits [M, V] in their storage type, labels [B, T] (the first loss rows' labels at column 0, V - 1 and the first column of the
    last slice, (V - 1) & ~7), and the kernel's two inputs as the fp32 rounding of the float64 forward: lse [M], coef [B] (stage 2, ratings 5 / 1)"""
    T = P + BL
    x = rnd(BB * T, V, seed=V + P, scale=2.0).to(BF if bf else F32)
    g = torch.Generator().manual_seed(V + 31 * P)
    lab = torch.randint(0, V, (BB, T), generator=g)
    lab[0, P + 1], lab[0, P + 2], lab[1, P + 1] = 0, V - 1, (V - 1) & ~7
    nll = _nll_ref(x.view(BB, T, V), lab)
    _, cf, _, _ = _sample_ref(nll, torch.tensor([5, 1]), 2, P, BL, float(BB))
    coef = (cf / ((BL - 1) * BB)).float()
    lse = _lse_ref(x).float()
    ex = (x.double() - lse.double()[:, None]).exp()
    ex.view(BB, T, V)[:, :-1].scatter_add_(-1, lab[:, 1:, None], -torch.ones(BB, T - 1, 1, dtype=torch.float64))
    return x, lab, lse, coef, ex          # ex = softmax - onehot of the rows, float64, from the fp32 lse the kernel is given


def _bwd_ref(V, P, bf, lm_coef, gscale):
    """float64 d(logits) [M, V] and the per-row factor: rc = gscale coef[b] on rows t >= P, + lm_coef on every row, 0 on a sample's
    last row; the fp32 values the kernel receives, as doubles"""
    x, lab, lse, coef, ex = _bwd_case(V, P, bf)
    T = P + BL
    t = torch.arange(BB * T) % T
    b = torch.arange(BB * T) // T
    rc = torch.where(t >= P, coef.double()[b] * float(np.float32(gscale)), torch.zeros((), dtype=torch.float64)) + float(np.float32(lm_coef))
    rc[t == T - 1] = 0.0
    return rc[:, None] * ex, rc


def _bwd_allow(d, rc, out_bf):
    """Every element is rc (expf(x - lse) - [label]) in fp32: the subtraction x - lse (rounded at its own magnitude, up to 24 here,
    so up to 24 2^-24 < 2^-21 relative on the exponential), expf, the label's 1, the product of coef and gscale, lm_coef's sum, the
    last product -- fewer than ten rounded operations, each moving the result by at most 2^-24 of |rc| max(exp, 1): 2^-20 |rc|
    absolute covers them with the exponent's share, 2^-20 |d| relative is for the last product.  A bf16 output is rounded once
    more, half an ulp = 2^-9 |d|; allowed 2^-8."""
    a = rc.abs()[:, None] * 2.0 ** -20 + d.abs() * 2.0 ** -20
    return a + d.abs() * 2.0 ** -8 if out_bf else a


def _bwd_check(name, got, V, Vpad, d, rc, allow, lm_coef, P, T):
    """got: [M, ldd] on the CPU.  Values, exact zeros of inactive rows and pad columns, the untouched columns, row sums"""
    g = got.double()
    _within(name, g[:, :V], d, allow)
    assert bool((got[:, V:Vpad] == 0).all()), name + ": columns [V, Vpad) must be exactly 0"
    assert bool((_bits(got[:, Vpad:]) == _bits(torch.full((1,), SENT, dtype=got.dtype))).all()), name + ": columns [Vpad, ldd) were written"
    t = torch.arange(got.shape[0]) % T
    inactive = (t == T - 1) | ((t < P) & (lm_coef == 0.0))
    assert bool((got[inactive][:, :Vpad] == 0).all()), name + ": an inactive row is not all zero"
    assert bool((got[~inactive][:, :V] != 0).any(1).all()), name + ": an active row is all zero"
    # softmax - onehot sums to zero over a row: the sum of what was written is the sum of its errors (and of the reference's own
    # sum, which is not 0 because the lse it is given is rounded to fp32)
    rows = g[:, :V].sum(1)
    assert bool((rows.abs() <= allow.sum(1) + d.sum(1).abs()).all()), name + ": row sums"


def _sentinel_out(M, Vpad, ldd, dtype):
    o = torch.full((M, ldd), NAN, dtype=dtype)
    o[:, Vpad:] = SENT
    return o


@gpu
@pytest.mark.parametrize("shape,form,P", _bwd_params())
def test_loss_bwd(shape, form, P):
    V, Vpad, ldd = shape
    T = P + BL
    M = BB * T
    in_bf = form.startswith("bf16")
    out_bf = form != "f32-f32"
    ldl = 336 if Vpad % 8 else ldd
    x, lab, lse, coef, _ = _bwd_case(V, P, in_bf)
    topic = lab[:, :P].contiguous().to(DEV) if P else None
    targ = lab[:, P:].contiguous().to(DEV)
    lsed, coefd = lse.to(DEV), coef.to(DEV)
    lg = torch.full((M, ldl), NAN, dtype=x.dtype)
    lg[:, :V] = x
    if form == "bf16-inplace":
        lg[:, Vpad:] = SENT
    for lm_coef in BWD_LM:
        for gscale in BWD_GS:
            name = "%s V=%d Vpad=%d ldd=%d P=%d lm_coef=%g gscale=%g" % (form, V, Vpad, ldd, P, lm_coef, gscale)
            d, rc = _bwd_ref(V, P, in_bf, lm_coef, gscale)
            lgd = lg.to(DEV)
            if form == "x3":
                pl = hip.Planes(torch.stack([_sentinel_out(M, Vpad, ldd, BF)] * 2).to(DEV), M, Vpad, ld=ldd)
                hip.loss_bwd_x3(lgd, ldl, V, topic, targ, lsed, coefd, gscale, BB, P, BL, pl, Vpad, lm_coef=lm_coef)
                plain = _sentinel_out(M, Vpad, ldd, BF).to(DEV)
                hip.loss_bwd(lgd, ldl, V, topic, targ, lsed, coefd, gscale, BB, P, BL, plain, ldd, Vpad, lm_coef=lm_coef)
                hi, lo = pl.t[0].cpu(), pl.t[1].cpu()
                # the hi plane is the fp32 -> bf16 entry's output (the same kernel instantiation), the lo plane what it dropped
                assert torch.equal(_bits(hi), _bits(plain.cpu())), name + ": hi plane differs from mmtg_loss_bwd's bf16 output"
                _bwd_check(name + " hi", hi, V, Vpad, d, rc, _bwd_allow(d, rc, True), lm_coef, P, T)
                s = hi.double() + lo.double()
                # hi + lo: bf16(v) is within 2^-9 of v and lo within 2^-9 of what is left -- 2^-18; allowed 2^-16 |d| over the fp32 bound
                _within(name + " hi + lo", s[:, :V], d, _bwd_allow(d, rc, False) + d.abs() * 2.0 ** -16)
                t = torch.arange(M) % T
                inactive = (t == T - 1) | ((t < P) & (lm_coef == 0.0))
                assert bool((lo[inactive][:, :Vpad] == 0).all()) and bool((lo[:, V:Vpad] == 0).all()), name + ": lo plane zeros"
                assert bool((_bits(lo[:, Vpad:]) == _bits(torch.full((1,), SENT, dtype=BF))).all()), name + ": lo plane columns [Vpad, ldd) were written"
                continue
            if form == "bf16-inplace":
                out = lgd
            else:
                out = _sentinel_out(M, Vpad, ldd, BF if out_bf else F32).to(DEV)
            hip.loss_bwd(lgd, ldl, V, topic, targ, lsed, coefd, gscale, BB, P, BL, out, ldd, Vpad, lm_coef=lm_coef)
            _bwd_check(name, out.cpu(), V, Vpad, d, rc, _bwd_allow(d, rc, out_bf), lm_coef, P, T)


@gpu
def test_loss_bwd_x3_rejects_a_lo_plane_in_front_of_the_hi_plane():
    V, Vpad, ldd, P = 333, 384, 384, 0
    M = BB * BL
    x, lab, lse, coef, _ = _bwd_case(V, P, False)
    lg = torch.zeros(M, ldd)
    lg[:, :V] = x
    t = torch.zeros(2, M, ldd, dtype=BF, device=DEV)
    args = (lg.to(DEV), ldd, V, None, lab.to(DEV), lse.to(DEV), coef.to(DEV), 1.0, BB, P, BL)
    with pytest.raises(RuntimeError, match="lo plane"):
        hip.loss_bwd_x3(*args, hip.Planes(t[1], M, Vpad, ld=ldd, plane=-M * ldd), Vpad)
    with pytest.raises(RuntimeError, match="lo plane"):        # planes that overlap: the lo plane one row early
        hip.loss_bwd_x3(*args, hip.Planes(t, M, Vpad, ld=ldd, plane=(M - 1) * ldd), Vpad)
    assert float(t.float().abs().max()) == 0.0


def test_loss_bwd_float32_restatement_cpu():
    """the bound of section 3 holds for the float32 CPU restatement of the kernel's expression on the same inputs (fp32 and bf16
    logits, both output types, every shape, P, lm_coef and gscale)"""
    for V in sorted({s[0] for s in BWD_SHAPES}):
        for P in BWD_P:
            for bf in (False, True):
                x, lab, lse, coef, _ = _bwd_case(V, P, bf)
                T = P + BL
                t = torch.arange(BB * T) % T
                b = torch.arange(BB * T) // T
                oh = torch.zeros(BB * T, V)
                oh.view(BB, T, V)[:, :-1].scatter_(-1, lab[:, 1:, None], 1.0)
                for lm_coef in BWD_LM:
                    for gscale in BWD_GS:
                        d, rc = _bwd_ref(V, P, bf, lm_coef, gscale)
                        cf = torch.where(t >= P, coef[b] * torch.tensor(gscale, dtype=F32), torch.zeros(())) + torch.tensor(lm_coef, dtype=F32)
                        cf[t == T - 1] = 0.0
                        d32 = cf[:, None] * (torch.exp(x.float() - lse[:, None]) - oh)
                        name = "float32 restatement V=%d P=%d bf=%s lm_coef=%g gscale=%g" % (V, P, bf, lm_coef, gscale)
                        _within(name, d32, d, _bwd_allow(d, rc, False))
                        _within(name + " (bf16 out)", d32.bfloat16(), d, _bwd_allow(d, rc, True))


# =====================================================================================================================
# 4. gradient norm
# =====================================================================================================================
SUMSQ_N = [1, 3, 4, 5, 1023, 262144, 262148, 2097152, 2097155, 2098179]


def _sumsq_call(x, n, out, ws):
    hip._check(hip.lib().mmtg_sumsq(x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "sumsq")


@gpu
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_exact(n):
    """integers in -2 .. 2: every partial sum is an integer below 4 n < 2^24, so the fp32 result is exact in any order -- a
    dropped or doubled element, tail, partial or workgroup changes it.  n crosses: scalar tail only (1, 3), no tail (4), both
    (5), one workgroup's worth (1023), 256 partials / 257 (262144 / 262148), the 2048-workgroup cap without and with a tail
    (2097152 / 2097155), a second trip of the grid-stride loop (2098179)."""
    assert 4 * n < 2 ** 24
    g = torch.Generator().manual_seed(n)
    x = torch.randint(-2, 3, (n,), generator=g)
    ref = int((x * x).sum())
    xd = x.float().to(DEV)
    need = int(hip.lib().mmtg_sumsq_ws(n))
    assert need == min(2048, (n // 4 + 1 + 255) // 256)
    ws = torch.full((need,), NAN, device=DEV)
    out = torch.full((3,), SENT, device=DEV)
    _sumsq_call(xd, n, out[1:], ws)
    first = out.cpu()
    assert first[1].item() == ref, (first[1].item(), ref)
    assert first[0].item() == SENT and first[2].item() == SENT          # written (not accumulated), and nothing beside it
    assert bool(torch.isfinite(ws).all())
    _sumsq_call(xd, n, out[1:], ws)
    assert torch.equal(_bits(out.cpu()), _bits(first))
    with pytest.raises(RuntimeError, match="workspace"):          # one float short
        hip._check(hip.lib().mmtg_sumsq(xd.data_ptr(), n, out[1:].data_ptr(), ws.data_ptr(), need - 1, torch.cuda.current_stream().cuda_stream), "sumsq")
    assert torch.equal(_bits(out.cpu()), _bits(first))


# =====================================================================================================================
# 5. AdamW
# =====================================================================================================================
ADAM_SMALL_N = [1, 3, 4, 5, 1027]
ADAM_BIG_N = [2097152, 2097155, 2098179]
ADAM_STEPS = [1, 2, 1000]
ADAM_CFGS = [(wd, ns, gs, cnt) for wd in (0.0, 0.01, 0.1) for ns in ("none", "active", "inactive", "zero") for gs in (1.0, 0.25)
             for cnt in (None, 7.0)]
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, max_norm=1.0)
# sqrt(3e4) = 173: clipped at every grad_scale / count used here (173 * 0.25 / 7 = 6.2 > max_norm); sqrt(1e-4) = 0.01: never
NORMSQ = {"none": None, "active": 3.0e4, "inactive": 1.0e-4, "zero": 0.0}


def _adam_data(n, seed, steps):
    """p, and per step a gradient: |g| log-uniform in [1e-6, 10], exact zeros at every 7th element (index 3, 10, ...: with m = v = 0
    the update there must be exactly 0), and one sign per element over the steps, so that no element of m is a cancelling sum
    and "2^-20 relative" is meaningful for it"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    gs = []
    for _ in range(steps):
        mag = torch.exp(torch.rand(n, generator=g).double() * math.log(1e7) + math.log(1e-6)).float().clamp(1e-6, 10.0)
        gr = sign * mag
        gr[3::7] = 0.0
        gs.append(gr)
    return p, gs


def _adam_formula(f, p, g, m, v, wd, normsq, grad_scale, count, step):
    """the header's formula in the arithmetic f (np.float64: the reference; np.float32: the restatement of the kernel).  The
    hyper-parameters are the fp32 values the kernel receives.  Returns p, m, v and the update ss m / (sqrt(v) + eps)."""
    h = {k: np.float32(x) for k, x in ADAM_HP.items()}
    one = f(1.0)
    gsc = f(np.float32(grad_scale))
    if count is not None:
        gsc = gsc * (one / f(np.float32(count)))
    coef = gsc
    if normsq is not None:
        nrm = np.sqrt(f(np.float32(normsq))) * gsc
        coef = coef * min(one, f(h["max_norm"]) / (nrm + f(np.float32(1e-6))))
    b1, b2 = float(h["b1"]), float(h["b2"])
    ss = f(float(h["lr"]) * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step))      # the bias-corrected step size, in double
    gi = g.astype(f) * coef
    mi = f(h["b1"]) * m.astype(f) + (one - f(h["b1"])) * gi
    vi = f(h["b2"]) * v.astype(f) + (one - f(h["b2"])) * gi * gi
    upd = ss * (mi / (np.sqrt(vi) + f(h["eps"])))
    pi = p.astype(f) - upd
    if wd > 0:
        pi = pi - f(h["lr"]) * f(np.float32(wd)) * pi
    return pi, mi, vi, upd


def _adam_check(name, before, g, after, wd, normsq, grad_scale, count, step):
    """one step judged alone: the float64 formula on the fp32 state the step started from.
    m and v: three or four rounded fp32 operations on top of the gradient's scaling (g coef, coef itself a handful of scalar
    roundings): 2^-20 relative is 16 of them.  p: the update's factors (m, sqrt(v) + eps, the quotient, the step size: each within
    a few 2^-24) give 2^-20 of the update; the difference p - update and the decoupled decay p - lr wd p are one correctly rounded
    operation each at the magnitude of p: 2^-23 |p|.  Division and square root are correctly rounded (no fast-math in build.py)."""
    p0, m0, v0 = (t.numpy() for t in before)
    pr, mr, vr, upd = _adam_formula(np.float64, p0, g.numpy(), m0, v0, wd, normsq, grad_scale, count, step)
    p1, m1, v1 = after
    _within(name + " m", m1, torch.from_numpy(mr), torch.from_numpy(np.abs(mr)) * 2.0 ** -20)
    _within(name + " v", v1, torch.from_numpy(vr), torch.from_numpy(np.abs(vr)) * 2.0 ** -20)
    _within(name + " p", p1, torch.from_numpy(pr), torch.from_numpy(np.abs(pr) * 2.0 ** -23 + np.abs(upd) * 2.0 ** -20))
    z = (g == 0) & (before[1] == 0) & (before[2] == 0)
    if wd == 0:
        assert torch.equal(_bits(p1[z]), _bits(before[0][z])), name + ": a zero gradient on zero state moved p"
    assert bool((m1[z] == 0).all()) and bool((v1[z] == 0).all()), name


def _adam_run(n, data, cfg, planes, offset, steps, state=None):
    """run the steps on the device; offset "p": the parameters start one float past a 16-byte boundary, "pc": the bf16 copy one
    bf16 past an 8-byte boundary (either sends every element down the scalar path).  planes: 0 no copy, 1 p_bf16, 2 p_bf16 and p_lo.
    Returns the (p, m, v, p_bf16, p_lo) on the CPU after every step."""
    wd, ns, gs, cnt = cfg
    p, grads = data
    dp = torch.zeros(n + 8, device=DEV)
    po = 1 if offset == "p" else 0
    dp = dp[po:po + n]
    dp.copy_(p)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    if state is not None:
        m.copy_(state[0])
        v.copy_(state[1])
    co = 1 if offset == "pc" else 0
    pc = torch.full((n + 8,), NAN, device=DEV, dtype=BF)[co:co + n] if planes >= 1 else None
    pl = torch.full((n + 8,), NAN, device=DEV, dtype=BF)[:n] if planes >= 2 else None
    assert dp.data_ptr() % 16 == 4 * po and (pc is None or pc.data_ptr() % 8 == 2 * co)
    nsd = None if NORMSQ[ns] is None else torch.tensor([NORMSQ[ns]], device=DEV)
    cd = None if cnt is None else torch.tensor([cnt], device=DEV)
    out = []
    for step, g in zip(steps, grads):
        hip.adamw(dp, g.to(DEV), m, v, pc, n, ADAM_HP["lr"], ADAM_HP["b1"], ADAM_HP["b2"], ADAM_HP["eps"], wd, step, nsd, ADAM_HP["max_norm"],
                  grad_scale=gs, count=cd, p_lo=pl)
        out.append(tuple(None if t is None else t.cpu() for t in (dp, m, v, pc, pl)))
    return out


def _adam_planes_check(name, res):
    p, _, _, pc, pl = res
    if pc is not None:
        assert torch.equal(_bits(pc), _bits(p.bfloat16())), name + ": p_bf16 != bf16(p)"
    if pl is not None:
        assert torch.equal(_bits(pl), _bits((p - pc.float()).bfloat16())), name + ": p_lo != bf16(p - float(p_bf16))"


def _adam_same_bits(name, a, b):
    for what, s, t in zip(("p", "m", "v", "p_bf16", "p_lo"), a, b):
        if s is not None and t is not None:
            assert torch.equal(_bits(s), _bits(t)), "%s: %s of the scalar path differs from the vector path" % (name, what)


@gpu
@pytest.mark.parametrize("n", ADAM_SMALL_N)
def test_adamw_three_steps(n):
    for i, cfg in enumerate(ADAM_CFGS):
        wd, ns, gs, cnt = cfg
        data = _adam_data(n, 100 * n + i, 3)
        planes = i % 3
        name = "n=%d wd=%g normsq=%s grad_scale=%g count=%s" % (n, wd, ns, gs, cnt)
        res = _adam_run(n, data, cfg, planes, None, ADAM_STEPS)
        before = (data[0], torch.zeros(n), torch.zeros(n))
        for step, g, r in zip(ADAM_STEPS, data[1], res):
            _adam_check("%s step %d" % (name, step), before, g, r[:3], wd, NORMSQ[ns], gs, cnt, step)
            _adam_planes_check("%s step %d" % (name, step), r)
            before = r[:3]
        for offset in ("p", "pc"):
            alt = _adam_run(n, data, cfg, max(planes, 1) if offset == "pc" else planes, offset, ADAM_STEPS)
            for step, r, a in zip(ADAM_STEPS, res, alt):
                _adam_same_bits("%s step %d offset %s" % (name, step, offset), r, a)
                _adam_planes_check("%s step %d offset %s" % (name, step, offset), a)


@gpu
@pytest.mark.parametrize("n", ADAM_BIG_N)
def test_adamw_past_the_grid(n):
    """2048 workgroups of 1024 parameters: the last full grid, a scalar tail behind it, and a second trip of the grid-stride loop;
    one step (number 2) from a non-zero state, both plane copies, and the all-scalar path on the same data"""
    cfg = (0.01, "active", 0.25, 7.0)
    p, (g, g2) = _adam_data(n, n, 2)
    state = (0.1 * g2, 1e-3 * g2 * g2)
    res = _adam_run(n, (p, [g]), cfg, 2, None, [2], state)[0]
    _adam_check("n=%d" % n, (p,) + state, g, res[:3], cfg[0], NORMSQ[cfg[1]], cfg[2], cfg[3], 2)
    _adam_planes_check("n=%d" % n, res)
    alt = _adam_run(n, (p, [g]), cfg, 2, "p", [2], state)[0]
    _adam_same_bits("n=%d offset p" % n, res, alt)


@gpu
@pytest.mark.parametrize("count", [0.0, -1.0, NAN])
@pytest.mark.parametrize("n", [5, 1027])
def test_adamw_skips_the_step_without_rows(n, count):
    """*count not greater than 0 (an empty global batch; NaN included): every buffer keeps its bits"""
    p, (g,) = _adam_data(n, n, 1)
    bufs = [p.to(DEV), rnd(n, seed=1).to(DEV), rnd(n, seed=2).abs().to(DEV), rnd(n, seed=3, dtype=BF).to(DEV), rnd(n, seed=4, dtype=BF).to(DEV)]
    keep = [b.clone() for b in bufs]
    hip.adamw(bufs[0], g.to(DEV), bufs[1], bufs[2], bufs[3], n, 1e-3, 0.9, 0.999, 1e-6, 0.01, 1, torch.tensor([3.0e4], device=DEV), 1.0,
              grad_scale=0.25, count=torch.tensor([count], device=DEV), p_lo=bufs[4])
    for b, k in zip(bufs, keep):
        assert torch.equal(_bits(b), _bits(k))


@gpu
def test_adamw_rejects_a_lo_plane_without_the_hi_plane():
    n = 8
    z = [torch.zeros(n, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError, match="lo plane"):
        hip.adamw(z[0], z[1], z[2], z[3], None, n, 1e-3, 0.9, 0.999, 1e-6, 0.0, 1, None, 1.0, p_lo=torch.zeros(n, device=DEV, dtype=BF))


def test_adamw_float32_restatement_cpu():
    """the bounds of section 5 hold for a numpy float32 restatement of the kernel's expression carried over the three steps, on
    the inputs of test_adamw_three_steps and test_adamw_past_the_grid"""
    for n in ADAM_SMALL_N:
        for i, cfg in enumerate(ADAM_CFGS):
            wd, ns, gs, cnt = cfg
            p, grads = _adam_data(n, 100 * n + i, 3)
            before = (p, torch.zeros(n), torch.zeros(n))
            for step, g in zip(ADAM_STEPS, grads):
                r = _adam_formula(np.float32, *(t.numpy() for t in (before[0], g, before[1], before[2])), wd, NORMSQ[ns], gs, cnt, step)
                after = tuple(torch.from_numpy(a) for a in r[:3])
                assert all(a.dtype == F32 for a in after)
                _adam_check("float32 restatement n=%d cfg %s step %d" % (n, cfg, step), before, g, after, wd, NORMSQ[ns], gs, cnt, step)
                before = after
    for n in ADAM_BIG_N[-1:]:
        cfg = (0.01, "active", 0.25, 7.0)
        p, (g, g2) = _adam_data(n, n, 2)
        state = (0.1 * g2, 1e-3 * g2 * g2)
        r = _adam_formula(np.float32, p.numpy(), g.numpy(), state[0].numpy(), state[1].numpy(), cfg[0], NORMSQ[cfg[1]], cfg[2], cfg[3], 2)
        _adam_check("float32 restatement n=%d" % n, (p,) + state, g, tuple(torch.from_numpy(a) for a in r[:3]), cfg[0], NORMSQ[cfg[1]], cfg[2], cfg[3], 2)


# =====================================================================================================================
# 6. slab sum, casts, axpy
# =====================================================================================================================
def _ints(shape, seed, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


@gpu
@pytest.mark.parametrize("n,splits_list", [(4, [1, 2, 3, 4, 5, 8, 9]), (1024, [1, 2, 3, 4, 5, 8, 9]), (8390656, [2])],
                         ids=["n4", "n1024", "past-8192-workgroups"])
def test_slab_sum_exact(n, splits_list):
    """integer slabs: the ordered fp32 sum is exact, so == decides.  splits cover the 4-way unrolled body alone (4, 8), its
    remainder alone (1, 2, 3) and both (5, 9); stride = n and n + 8 (NaN between the slabs); n = 8390656 is 8194 workgroups of 1024
    floats against the cap of 8192"""
    for splits in splits_list:
        for stride in (n, n + 8):
            part = torch.full((splits, stride), NAN)
            part[:, :n] = _ints((splits, n), n + splits)
            ref = torch.zeros(n)
            for s in range(splits):
                ref = ref + part[s, :n]
            pd = part.to(DEV)
            for acc in (0, 1):
                dst = torch.full((n + 16,), NAN if acc == 0 else 0.0)
                prior = _ints((n,), 5 * n + splits)
                if acc:
                    dst[:n] = prior
                dst[n:] = SENT
                dd = dst.to(DEV)
                hip.slab_sum(pd, splits, stride, dd, n, accumulate=bool(acc))
                got = dd.cpu()
                name = "n=%d splits=%d stride=%d accumulate=%d" % (n, splits, stride, acc)
                assert torch.equal(got[:n], ref + prior if acc else ref), name
                assert bool((got[n:] == SENT).all()), name + ": dst[n:] was written"


def _same(got, ref):
    """bit for bit, except that a NaN need only stay a NaN (its payload is not pinned)"""
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return torch.equal(gn, rn) and torch.equal(_bits(got)[~gn], _bits(ref)[~rn])


CAST_N = [1, 524288, 524291]        # one element; 2048 workgroups exactly; past them (a second trip of the grid-stride loop)


def _cast_src(n):
    pats = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000,
                     0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x807FFFFF,
                     0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001],
                    dtype=np.uint32)
    src = rnd(n, seed=n)
    k = min(n, len(pats))
    src[n - k:] = torch.from_numpy(pats[:k].view(np.float32).copy())      # the table at the END: the last elements of the last trip
    if n > 2 * len(pats):
        src[:len(pats)] = torch.from_numpy(pats.view(np.float32).copy())
    return src


@gpu
@pytest.mark.parametrize("n", CAST_N)
def test_casts_exact(n):
    """fp32 -> bf16 is round-to-nearest-even exactly as torch does it on the table of _cast_src (ties both ways, zeros,
    subnormals, overflow to inf, inf, NaN stays NaN); fp32 -> fp32 and bf16 -> fp32 keep every bit; for n >= 65536 the bf16 source
    holds every one of the 65536 bf16 values"""
    src = _cast_src(n)
    sd = src.to(DEV)
    for dtype in (BF, F32):
        dst = torch.full((n + 8,), SENT, device=DEV, dtype=dtype)
        hip.cast_f32_to(sd, dst, n)
        got = dst.cpu()
        assert _same(got[:n], src.to(dtype)), "cast_f32_to %s n=%d" % (dtype, n)
        assert bool((got[n:] == SENT).all())
    b = src.bfloat16()
    if n >= 65536:
        b[:65536] = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF)
    for s in (b, src):
        dst = torch.full((n + 8,), SENT, device=DEV)
        hip.cast_to_f32(s.to(DEV), dst, n)
        got = dst.cpu()
        assert _same(got[:n], s.float()), "cast_to_f32 %s n=%d" % (s.dtype, n)
        assert bool((got[n:] == SENT).all())


@gpu
@pytest.mark.parametrize("n", CAST_N)
def test_axpy_exact(n):
    """y += 3 x on small integers: exact whether or not the product and the sum are fused"""
    x, y = _ints((n,), n), _ints((n,), n + 1)
    yd = torch.full((n + 8,), SENT, device=DEV)
    yd[:n] = y.to(DEV)
    hip.axpy_f32(yd, x.to(DEV), 3.0, n)
    got = yd.cpu()
    assert torch.equal(got[:n], y + 3.0 * x)
    assert bool((got[n:] == SENT).all())


@gpu
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_cast_pad_rows(dtype):
    """rows of 530 columns out of a source of stride 540 (NaN in its padding) into rows of 600: three passes of the 256 threads,
    the cast exact, the padding exactly 0, nothing written behind the last row"""
    rows, cols, lds, ldd = 5, 530, 540, 600
    src = torch.full((rows, lds), NAN)
    src[:, :cols] = rnd(rows, cols, seed=9)
    src[0, :26] = _cast_src(26)
    dst = torch.full((rows + 1, ldd), NAN, device=DEV, dtype=dtype)
    dst[rows] = SENT
    hip.cast_pad_rows(src.to(DEV), lds, dst, ldd, rows, cols)
    got = dst.cpu()
    assert _same(got[:rows, :cols], src[:, :cols].to(dtype))
    assert torch.equal(_bits(got[:rows, cols:]), torch.zeros(rows, ldd - cols, dtype=_bits(got).dtype))
    assert bool((got[rows] == SENT).all())
