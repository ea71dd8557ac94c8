"""Token-level unlikelihood on repeated lyric tokens: the float64 reference of the rule in include/mmtg_hip.h, the error bounds of its
fp32 evaluation, and a float32 restatement of the kernels' expressions (csrc/loss.hip: ul_row_kernel, ul_sample_kernel,
loss_bwd_ul_kernel).

Convention (as tests/test_train_ops_gpu.py's _bwd_case): torch on the CPU; the logits come in their storage type and are widened
exactly; lse is the fp32 row log-sum-exp the kernel is given, widened exactly; so are coef, S (for the backward), gscale, lm_coef and u.

The bounds, derived by counting rounded fp32 operations (eps = 2^-24 is half an ulp relative, TR = 2^-21 covers a transcendental:
OpenCL's full-profile bound for exp and log is 3 ulp <= 3 * 2^-23 < 2^-21; HIP's fp32 division is correctly rounded):

  a = x - lse      one rounding: |da| <= eps |a|
  p = exp(a)       dp = p (eps |a| + TR)                                   (the exponent's error is relative on p)
  q = 1 - p        dq = dp + eps q                                          (p's error is ABSOLUTE on q: the 1 / (1 - p) amplification)
  -log q           dterm = -log(1 - dq / q) + TR |log q|                    (exact perturbation of the log, not first order)
  g = p / q        dg = (p + dp) / (q - dq) - p / q + eps g                 (exact perturbation of the quotient: dq / q again)
  a sum of n terms of one sign, in ANY order: (n - 1) eps * the sum on top of the terms' own errors
  a clamped candidate (q < UL_FLOOR): the term is -logf(1e-5f), TR |log| allowed; g is exactly 0.  The case builder keeps every
  candidate's q outside [UL_FLOOR / 2, 2 UL_FLOOR], far more than dq, so reference and kernel clamp the same candidates.

  d[m, v] = t1 + t2 + t3,  t1 = cf (p - [label]),  t2 = -(u S) p,  t3 = u [v in C] g
  t1: section 3 of tests/test_train_ops_gpu.py: 2^-20 |cf| + 2^-20 |t1| (it takes |a| <= 24; |cf| dp covers the rows planted here with
      a dominating logit, |a| up to 45);  t2: |u S| (dp + 2 eps p) (the product u S, the product with p);  t3: u (dg + 2 eps g);
  the two additions (or one fused multiply-add): 2 eps (|t1| + |t2| + |t3|).
  A bf16 output is rounded once more: half an ulp, at most 2^-8 |d|; hi + lo of a plane pair: 2^-16 |d| (each part within 2^-8 of
  what it rounds).
"""
import numpy as np
import torch

UL_FLOOR = float(np.float32(1e-5))
EPS = 2.0 ** -24
TR = 2.0 ** -21
F64 = torch.float64
DEFAULT_EXCLUDE = (0, 1, 2, 100, 102)


def candidate_mask(targets, P, V, exclude):
    """bool [B * (P + L), V]: the candidate set of every loss row (all False elsewhere).  targets: int64 [B, L] as given (ids outside
    [0, V) included)."""
    tg = np.asarray(targets)
    B, L = tg.shape
    Tt = P + L
    mask = np.zeros((B * Tt, V), dtype=bool)
    ex = np.asarray(sorted(set(int(e) for e in (exclude or ()))), dtype=np.int64)
    for b in range(B):
        for j in range(1, L):
            ids = np.unique(tg[b, :j])
            ids = ids[(ids >= 0) & (ids < V) & (ids != tg[b, j])]
            if ex.size:
                ids = ids[~np.isin(ids, ex)]
            mask[b * Tt + P + j - 1, ids] = True
    return torch.from_numpy(mask)


def loss_rows(B, P, L):
    """bool [M]: the rows that carry the term, P <= t <= Tt - 2"""
    t = torch.arange(B * (P + L)) % (P + L)
    return (t >= P) & (t <= P + L - 2)


def forward(x, lse, targets, P, V, exclude, batch_den):
    """x: [M, >= V] logits in their storage type, lse fp32 [M].  Returns a dict of float64 tensors: p, dp [M, V]; mask; term, g and
    their bounds dterm, dg [M, V] (0 outside the mask); ul_row, S [M] and allow_row, allow_S; ul_sample [B], ul [] and their bounds
    (for a sample kernel fed with values inside allow_row); n [M] candidates per row."""
    B, L = targets.shape
    Tt = P + L
    ntok = Tt - 1 - P
    mask = candidate_mask(targets, P, V, exclude)
    a = x[:, :V].to(F64) - lse.to(F64)[:, None]
    p = a.exp()
    dp = p * (EPS * a.abs() + TR)
    q = 1.0 - p
    dq = dp + EPS * q.abs()
    qc = torch.where(mask, q, torch.ones_like(q))                   # (outside the mask: harmless values)
    dqc = torch.where(mask, dq, torch.zeros_like(q))
    clamped = mask & (q < UL_FLOOR)
    near = mask & (q > 0.5 * UL_FLOOR) & (q < 2.0 * UL_FLOOR)
    assert not bool(near.any()), "a candidate's 1 - p is too close to UL_FLOOR for a test: %s" % q[near]
    live = mask & ~clamped
    safe_q = torch.where(live, qc, torch.ones_like(q))
    safe_dq = torch.where(live, dqc, torch.zeros_like(q))
    assert bool((safe_dq < 0.5 * safe_q).all())
    pl = torch.where(live, p, torch.zeros_like(p))
    dpl = torch.where(live, dp, torch.zeros_like(p))
    term = torch.where(live, -safe_q.log(), torch.zeros_like(q))
    dterm = torch.where(live, -(1.0 - safe_dq / safe_q).log() + TR * term.abs(), torch.zeros_like(q))
    g = pl / safe_q
    dg = (pl + dpl) / (safe_q - safe_dq) - g + EPS * g
    floor_term = -float(np.log(np.float64(UL_FLOOR)))
    term = torch.where(clamped, torch.full_like(q, floor_term), term)
    dterm = torch.where(clamped, torch.full_like(q, TR * floor_term), dterm)
    n = mask.sum(1).to(F64)
    ul_row, S = term.sum(1), g.sum(1)
    order = (n - 1).clamp(min=0) * EPS
    allow_row = dterm.sum(1) + order * ul_row + 1e-300
    allow_S = dg.sum(1) + order * S + 1e-300
    rows = loss_rows(B, P, L)
    assert not bool(mask[~rows].any())
    per = ul_row.view(B, Tt)[:, P:Tt - 1]
    ul_sample = per.sum(1) / ntok
    allow_sample = (allow_row.view(B, Tt)[:, P:Tt - 1].sum(1) + (ntok - 1) * EPS * per.sum(1)) / ntok + EPS * ul_sample + 1e-300
    den = float(np.float32(batch_den))
    ul = ul_sample.sum() / den
    allow_ul = allow_sample.sum() / den + (B + 1) * EPS * ul + 1e-300
    return dict(mask=mask, p=p, dp=dp, q=q, clamped=clamped, term=term, dterm=dterm, g=g, dg=dg, n=n, ul_row=ul_row, S=S,
                allow_row=allow_row, allow_S=allow_S, ul_sample=ul_sample, allow_sample=allow_sample, ul=ul, allow_ul=allow_ul)


def clamp_labels(topic, targets, V):
    """labels [B, Tt] as the loss kernels read them: cat(topic, targets) clamped into [0, V)"""
    lab = targets if topic is None else torch.cat([topic, targets], 1)
    return lab.clamp(0, V - 1)


def row_factor(coef, gscale, lm_coef, B, P, L):
    """float64 [M]: cf of mmtg_loss_bwd from the fp32 values the kernel receives; 0 on a sample's last row"""
    Tt = P + L
    m = torch.arange(B * Tt)
    t, b = m % Tt, m // Tt
    rc = torch.where(t >= P, coef.to(F64)[b] * float(np.float32(gscale)), torch.zeros((), dtype=F64)) + float(np.float32(lm_coef))
    rc[t == Tt - 1] = 0.0
    return rc


def backward(fw, S32, topic, targets, coef, gscale, lm_coef, u, P, V):
    """float64 d(logits) [M, V] and its fp32 bound, from forward()'s dict and the fp32 S the kernel is given.  Rows without the term are
    mmtg_loss_bwd's."""
    B, L = targets.shape
    rows = loss_rows(B, P, L).to(F64)
    rc = row_factor(coef, gscale, lm_coef, B, P, L)
    lab = clamp_labels(topic, targets, V)
    oh = torch.zeros_like(fw["p"])
    oh.view(B, P + L, V)[:, :-1].scatter_(-1, lab[:, 1:, None], 1.0)
    uf = float(np.float32(u))
    us = (uf * S32.to(F64) * rows)[:, None]
    t1 = rc[:, None] * (fw["p"] - oh)
    t2 = -us * fw["p"]
    t3 = uf * fw["g"]                       # (0 outside the candidate sets, hence outside the loss rows)
    d = t1 + t2 + t3
    allow = (rc.abs()[:, None] * (2.0 ** -20 + fw["dp"]) + t1.abs() * 2.0 ** -20 + us.abs() * (fw["dp"] + 2 * EPS * fw["p"])
             + uf * (fw["dg"] + 2 * EPS * fw["g"]) + 2 * EPS * (t1.abs() + t2.abs() + t3.abs()))
    return d, allow, rc


def out_allow(d, allow, form):
    """the bound for an output stored as fp32 / bf16 / the sum of a (hi | lo) pair"""
    if form == "f32":
        return allow
    return allow + d.abs() * (2.0 ** -8 if form == "bf16" else 2.0 ** -16)


# ---- the kernels' expressions in float32 (torch on the CPU): what the bounds must admit
def forward32(x, lse, targets, P, V, exclude, batch_den):
    f = torch.float32
    B, L = targets.shape
    Tt = P + L
    mask = candidate_mask(targets, P, V, exclude)
    p = torch.exp(x[:, :V].to(f) - lse[:, None])
    q = 1.0 - p
    live = mask & (q >= np.float32(UL_FLOOR))
    clamped = mask & ~live
    one = torch.ones_like(q)
    term = torch.where(live, -torch.log(torch.where(live, q, one)), torch.zeros_like(q))
    term = torch.where(clamped, -torch.log(torch.full_like(q, UL_FLOOR)), term)
    g = torch.where(live, p / torch.where(live, q, one), torch.zeros_like(q))
    ul_row, S = term.sum(1), g.sum(1)
    ul_sample = ul_row.view(B, Tt)[:, P:Tt - 1].sum(1) / np.float32(Tt - 1 - P)
    ul = ul_sample.sum() / np.float32(batch_den)
    return dict(mask=mask, p=p, g=g, ul_row=ul_row, S=S, ul_sample=ul_sample, ul=ul)


def backward32(f32, S32, topic, targets, coef, gscale, lm_coef, u, P, V):
    f = torch.float32
    B, L = targets.shape
    Tt = P + L
    m = torch.arange(B * Tt)
    t, b = m % Tt, m // Tt
    cf = torch.where(t >= P, coef[b] * torch.tensor(gscale, dtype=f), torch.zeros((), dtype=f)) + torch.tensor(lm_coef, dtype=f)
    cf[t == Tt - 1] = 0.0
    lab = clamp_labels(topic, targets, V)
    oh = torch.zeros_like(f32["p"])
    oh.view(B, Tt, V)[:, :-1].scatter_(-1, lab[:, 1:, None], 1.0)
    uf = torch.tensor(u, dtype=f)
    us = torch.where(loss_rows(B, P, L), uf * S32, torch.zeros((), dtype=f))[:, None]
    return cf[:, None] * (f32["p"] - oh) - us * f32["p"] + uf * f32["g"]


# ---- the cases of tests/test_ul_ops_gpu.py (built once per process; the CPU yardstick of tests/test_ul_cpu.py walks the same list)
import functools  # noqa: E402

B = 2
SHAPES = [(333, 336, 336), (333, 384, 400), (16392, 16392, 16392)]          # V, Vpad, ld: with L in SHORT_L
SHORT_L = [3, 66]
LONG_SHAPE = (333, 384, 384)                                                # with L in LONG_L: the wave and workgroup edges of the context loop
LONG_L = [258, 1024]
SCALAR_SHAPE = (333, 335, 335)      # (an addition to the issue's list: Vpad % 8 != 0 takes the kernel's scalar dense pass; rows of stride 336)
PS = [0, 3]
U = 0.3
COMBOS = [(0.0, 1.0), (0.37, 1.0 / 7.0)]            # (lm_coef, gscale)


def geometries():
    """(V, Vpad, ld, L) of every case"""
    out = [s + (L,) for s in SHAPES for L in SHORT_L]
    out += [LONG_SHAPE + (L,) for L in LONG_L]
    out.append(SCALAR_SHAPE + (3,))
    return out


def _raise_logit(x, m, c, V, one_minus_p):
    """set x[m, c] so that p(c) = 1 - one_minus_p on the row as stored (float64 arithmetic, then the storage type's rounding)"""
    row = x[m, :V].to(F64)
    row[c] = -float("inf")
    x[m, c] = float(torch.logsumexp(row, 0) + np.log((1.0 - one_minus_p) / one_minus_p))


@functools.lru_cache(maxsize=None)
def case(V, P, L, bf):
    """Logits [M, V] in their storage type (scale-2 normal), topic [B, P] / targets [B, L] with the planted ids, and the backward's
    fp32 inputs: lse [M] (the fp32 rounding of the float64 row log-sum-exp), coef [B].  `planted` names the rows (m) that hold each
    planted situation, for the tests to assert they are there.

    L >= 66 holds every planted case.  L = 3 has two loss rows per sample and contexts of one and two ids: it holds a doubled id (the
    context cannot hold three), the label in the context (an empty set), an excluded id, candidates at 0, V - 1 and (V - 1) & ~7, the
    clamped and the near-1e-3 candidate; an id outside [0, V) does not fit beside them."""
    Tt = P + L
    M = B * Tt
    gen = torch.Generator().manual_seed(1000 * V + 10 * L + P)
    x = (torch.randn(M, V, generator=gen) * 2.0).to(torch.bfloat16 if bf else torch.float32)
    pool = torch.tensor([i for i in range(3, min(V, 300)) if i not in DEFAULT_EXCLUDE])       # 300 .. 310 are kept for planting
    tg = pool[torch.randint(0, len(pool), (B, L), generator=gen)]
    topic = pool[torch.randint(0, len(pool), (B, P), generator=gen)] if P else None
    last8 = (V - 1) & ~7
    row = lambda b, j: b * Tt + P + j - 1           # the row that predicts targets[b, j]
    pl = {}
    if L == 3:
        tg[0] = torch.tensor([V - 1, V - 1, 7])       # j = 1: the label is the context (empty);  j = 2: V - 1 twice, one candidate
        tg[1] = torch.tensor([0, last8, 9])           # j = 1: PAD alone (empty by default, column 0 without a list);  j = 2: 0 and last8
        pl.update(dup=row(0, 2), label_in_context=row(0, 1), empty=row(0, 1), excluded=row(1, 1), near=(row(0, 2), V - 1),
                  clamped=(row(1, 2), last8))
    else:
        A = 301
        tg[0, 0] = tg[0, 3] = tg[0, 7] = A            # three times: once
        tg[0, 10] = tg[0, 4]                          # the label of row j = 10 is in its context
        tg[0, 11:16] = torch.tensor(DEFAULT_EXCLUDE)
        tg[0, 16], tg[0, 17], tg[0, 18] = V, -3, V + 70000
        tg[0, 19], tg[0, 20], tg[0, 21] = V - 1, last8, 0
        tg[1, 0] = -7                                 # row j = 1 of sample 1: nothing in range, an empty set with or without a list
        tg[1, 5], tg[1, 6] = 302, 303
        pl.update(dup=row(0, 8), label_in_context=row(0, 10), empty=row(1, 1), excluded=row(0, 16), out_of_range=row(0, 19),
                  near=(row(1, L - 2), 302), clamped=(row(1, L - 1), 303))
        if L >= 258:      # ids whose first occurrence sits at the edges of the 256-thread trips and the 64-lane waves
            for k, i in enumerate(i for i in (63, 64, 255, 256, 511, 512, 767, 768, L - 2) if i < L - 1):
                tg[0, i] = 304 + k
    _raise_logit(x, pl["near"][0], pl["near"][1], V, 1e-3)
    xm = pl["clamped"][0]
    x[xm, pl["clamped"][1]] = float(x[xm, :V].float().max()) + 25.0        # 1 - p about V e^-25: clamped
    lse = torch.logsumexp(x[:, :V].to(F64), 1).float()
    ntok = L - 1
    coef = (torch.tensor([0.8, -0.35], dtype=F64) / (ntok * B)).float()
    return x, topic, tg, lse, coef, pl


@functools.lru_cache(maxsize=None)
def reference(V, P, L, bf, with_list):
    """forward() of the case, with the default exclude list or none"""
    x, topic, tg, lse, coef, pl = case(V, P, L, bf)
    return forward(x, lse, tg, P, V, DEFAULT_EXCLUDE if with_list else None, float(B))
