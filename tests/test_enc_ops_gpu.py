"""The multi-modal front end, one entry at a time, against float64 restatements (csrc/encoder.hip, csrc/embed.hip).

tests/test_ops_gpu.py runs these fourteen entries at H = 512 with natural strides, zeroed accumulators and tolerances that grow with
the reduction length: a kernel that ignored a stride, wrote the next step's rows, overwrote where it must add or dropped a lane
tail passes it.  Here every case hands ONE entry inputs already rounded to its storage type (fp32 and bf16), starts every output as
NaN between sentinel pads (accumulating outputs at small integers), puts NaN rows behind every operand in the same allocation, and
compares what the entry wrote with the same operation restated in float64 on the CPU; every element the entry has no business with
-- pads, the neighbouring steps of a strided buffer, unreferenced rows, the operands themselves -- must come back bit-identical.

  1. recurrent cells (mmtg_gru_cell_fwd / bwd / bwd_fused, mmtg_rnn_cell_fwd / bwd as LSTM and ReLU-RNN): natural strides, the
     engine's batch-first step form (step 1 of a [B, 3, *] buffer), ld_gh = 0, null h_prev / c_prev / carry / part; random,
     saturated and signed-zero pre-activations; the backward on dyadic `save` planes bit for bit, on random ones to the bound;
  2. alpha attention (mmtg_alpha_attn_fwd / bwd): every S = 1 .. 8, head widths 8 .. 320, kl on a non-zero start, exact, peaked and
     random scores, the backward on the probs the forward stored;
  3. beta fuser (mmtg_beta_fuse_fwd / bwd): H = 8 .. 1024, S = 1 .. 16 (17 in the atomic form), the workspace form through
     hip.beta_fuse_bwd and the null-workspace atomic form through hip.lib(), accumulation onto start values;
  4. embedding front end (mmtg_embed_condition, mmtg_segment_sum, mmtg_embed_add, mmtg_embed_add_bwd in both finishes,
     mmtg_dropout_apply): sweep edges, id clamps, empty segments, the dropout mask as a function of (seed, m D + d);
  5. the argument sets each entry refuses: the error comes back and nothing is written.

One restatement of each kernel (k_* below) is written over an arithmetic that is either V -- float64 values carrying a first-order
error bound: U = 2^-24 per fp32 operation, the operands' errors through each operation's derivative, half an ulp of the storage
type per bf16 store, n U sum|terms| for a sum in unknown order -- or plain float32 tensors in the kernel's order (lane striding,
wave-sum tree, sequential segment / batch / slab sums, row blocks of 128, the strides as given).  The first is the reference and
its bound; the second is the CPU model the tests without the gpu mark run through the same checks on the same inputs -- a bound the
model cannot meet is a wrong derivation -- and in which twenty defects are planted, one at a time, each of which a named case must
REJECT.  Cases whose result is exact in fp32 whatever the order (integers, dyadic planes) are compared bit for bit with the float64
value rounded once to the storage type; the single-rounding outputs (embed_condition, embed_add, dropout_apply) with the fp32
operation sequence of the kernel.  Only the transcendental yardsticks are measured (test_enc_transcendental_yardsticks, beside
test_gemm_ops_gpu.test_transcendental_yardsticks; docs/experiments.md, "Encoder and embedding kernels against float64").

Left out on purpose: the 32-bit wrap of the dropout hash index (unreachable at a test's size), the bit patterns of the atomic
finishes (order-dependent; they are held to the summation bound), and the model-level paths the oracle tests already cover.
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import _hash_u32  # noqa: E402
import test_gemm_ops_gpu as G  # noqa: E402  (the shared helpers and the transcendental yardsticks)

gpu = pytest.mark.gpu

DEV, NAN, SENT, PAD, U = G.DEV, G.NAN, G.SENT, G.PAD, G.U
ARG_MAX, LIBM_FACTOR, TANH_YARD = G.ARG_MAX, G.LIBM_FACTOR, G.TANH_YARD
_cdiv, _half_ulp = G._cdiv, G._half_ulp
BF, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
POISON = 64                  # NaN elements behind every operand, in the same allocation
SEED = 4242                  # dropout seed
WORST = {}                   # family -> worst err / allowed seen in this process

# The measured terms (test_enc_transcendental_yardsticks prints the figures these constants come from): the largest error of the
# float32 form on the CPU against float64 over the arguments the cases produce; the kernels are allowed LIBM_FACTOR times it.
SIG_YARD = 8.6e-8            # absolute: 1 / (1 + exp(-x)), |x| <= ARG_MAX and +-100 (sigmoid_f; the fast exponential's |x| U is added in V.sig)
EXP_YARD = 6.1e-8            # of exp(x), SOFTMAX_ARG_MIN <= x <= 0 (the two softmaxes)
LOG_YARD = 5.2e-8            # of |log x|, LOG_ARG_MIN <= x <= 1 (the KL term)
SOFTMAX_ARG_MIN = -80.0      # (exp(-80) = 1.8e-35 is still a normal fp32 number)
LOG_ARG_MIN = 1e-30


def _T(bf):
    return BF if bf else F32


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.dtype == F32 else t


def _ar(n):
    return torch.arange(n, dtype=I64)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


def _pick(choices, *shape, seed):
    c = torch.tensor(choices, dtype=F32)
    return c[torch.randint(0, len(choices), shape, generator=_gen(seed))]


def _ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float()


# =====================================================================================================================
# the two arithmetics
# =====================================================================================================================
class V:
    """float64 values with a bound on what an fp32 evaluation of the same expression may be off by.  Every operation adds U |result|
    for its own rounding and passes its operands' bounds through its first derivative (plus the second-order product term)."""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def lift(x):
        if isinstance(x, V):
            return x
        x = torch.as_tensor(x, dtype=F64)
        assert bool((x.float().double() == x).all())        # constants are fp32 numbers
        return V(x)

    def __add__(self, o):
        o = V.lift(o)
        v = self.v + o.v
        return V(v, self.e + o.e + U * v.abs())

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.e)

    def __sub__(self, o):
        return self + (-V.lift(o))

    def __rsub__(self, o):
        return V.lift(o) + (-self)

    def __mul__(self, o):
        o = V.lift(o)
        v = self.v * o.v
        return V(v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + U * v.abs())

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.lift(o)
        v = self.v / o.v
        den = (o.v.abs() - o.e).clamp(min=1e-300)
        return V(v, (self.e + v.abs() * o.e) / den + U * v.abs())

    def __rtruediv__(self, o):
        return V.lift(o) / self

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    @property
    def shape(self):
        return self.v.shape

    def expand(self, *s):
        return V(self.v.expand(*s), self.e.expand(*s))

    def reshape(self, *s):
        return V(self.v.reshape(*s), self.e.reshape(*s))

    def sig(self):
        """sigmoid_f = 1 / (1 + __expf(-x)): the yardstick, the fast exponential's argument rounding |x| U (relative on the
        exponential, s (1 - s) of it on s), times the factor; the operand's error through s' <= s (1 - s) + e, at most 1 / 4"""
        s = torch.sigmoid(self.v)
        return V(s, LIBM_FACTOR * (SIG_YARD + self.v.abs() * U * s * (1 - s)) + self.e * (s * (1 - s) + self.e).clamp(max=0.25))

    def tanh(self):
        t = torch.tanh(self.v)
        return V(t, LIBM_FACTOR * TANH_YARD + self.e * (1 - t * t + 2 * self.e).clamp(max=1.0))

    def exp(self):
        assert bool((self.v >= SOFTMAX_ARG_MIN).all())
        x = torch.exp(self.v)
        return V(x, x * (torch.expm1(self.e) + LIBM_FACTOR * EXP_YARD))

    def log(self):
        assert bool((self.v >= LOG_ARG_MIN).all())
        x = torch.log(self.v)
        return V(x, self.e / (self.v - self.e).clamp(min=1e-300) + LIBM_FACTOR * LOG_YARD * x.abs())

    def relu(self):
        return V(self.v.clamp(min=0), self.e)


def fsig(x):
    return x.sig() if isinstance(x, V) else 1.0 / (1.0 + torch.exp(-x))


def ftanh(x):
    return x.tanh() if isinstance(x, V) else torch.tanh(x)


def fexp(x):
    return x.exp() if isinstance(x, V) else torch.exp(x)


def flog(x):
    return x.log() if isinstance(x, V) else torch.log(x)


def frelu(x):
    return x.relu() if isinstance(x, V) else x.clamp(min=0)


def fshift(xs):
    """the softmax shift: the largest of the scores, taken as a constant -- softmax is the same function for any shift"""
    if isinstance(xs[0], V):
        m = xs[0].v
        for x in xs[1:]:
            m = torch.maximum(m, x.v)
        return V(m)
    m = xs[0]
    for x in xs[1:]:
        m = torch.maximum(m, x)
    return m


def fwhere(mask, a, b):
    if isinstance(a, V) or isinstance(b, V):
        a, b = V.lift(a), V.lift(b)
        return V(torch.where(mask, a.v, b.v), torch.where(mask, a.e, b.e))
    return torch.where(mask, a, torch.as_tensor(b, dtype=F32))


def flanes(x, perm):
    return V(x.v[..., perm], x.e[..., perm]) if isinstance(x, V) else x[..., perm]


def wave_sum(x):
    """common.h wave_sum: six butterfly levels over the last (64-lane) axis; every lane ends with the same bits"""
    lanes = _ar(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + flanes(x, lanes ^ o)
    return x[..., 0]


class HB:
    """host image of one allocation: PAD sentinels | n elements | (operands: POISON NaN elements) | PAD sentinels.  base: where the
    pointer handed to the entry points (PAD + the offset of the step addressed); ld: the row stride that goes with it"""

    def __init__(self, n, dtype, fill, operand):
        self.dtype, self.n = dtype, n
        tail = POISON if operand else 0
        isf = dtype in (BF, F32)
        self.host = torch.full((PAD + n + tail + PAD,), fill if isf else -77777, dtype=dtype)
        self.host[:PAD] = SENT if isf else -99999
        self.host[PAD + n + tail:] = SENT if isf else -99999
        self.base, self.ld = PAD, None


def _rows(B, W, dtype, data=None, S=1, t=0, operand=None, start=NAN):
    """[B, S, W] with rows (b, t, :) addressed: an operand (data given) has NaN everywhere else, an output has sentinels in the
    other steps and `start` (NaN, or the values an accumulating output starts from) in the rows addressed"""
    operand = data is not None if operand is None else operand
    hb = HB(B * S * W, dtype, NAN if operand else SENT, operand)
    idx = PAD + (_ar(B)[:, None] * S + t) * W + _ar(W)[None, :]
    hb.host[idx] = torch.full((B, W), start, dtype=dtype) if data is None else data.reshape(B, W).to(dtype)
    hb.base, hb.ld = PAD + t * W, S * W
    return hb


def _vec(data, dtype=F32):
    return _rows(1, data.numel(), dtype, data.reshape(1, -1))


def _outv(n, dtype=F32, start=NAN):
    return _rows(1, n, dtype, None, start=start)


def _acc(start, dtype=F32):
    """an accumulating output holding `start` on entry"""
    return _rows(1, start.numel(), dtype, start.reshape(1, -1), operand=False)


class Ctx:
    """one evaluation of a restated kernel: reads of the host images, the list of writes.  ref: V arithmetic, else float32"""

    def __init__(self, ref, defect=None):
        self.ref, self.defect, self.recs = ref, defect, []

    def rd(self, hb, idx, valid=None):
        idx = torch.as_tensor(idx)
        if valid is not None:
            idx = torch.where(valid, idx, torch.zeros_like(idx))
        pos = (hb.base + idx).clamp(0, hb.host.numel() - 1)    # (a planted defect may point anywhere: it reads what lies there)
        x = hb.host[pos]
        x = x.double() if self.ref else x.float()
        if valid is not None:
            x = torch.where(valid, x, torch.zeros_like(x))
        return V(x) if self.ref else x

    def ids(self, hb, idx):
        return hb.host[(hb.base + torch.as_tensor(idx)).clamp(0, hb.host.numel() - 1)]

    def const(self, x64, roundings=1):
        """a value the kernel computes once in fp32 (rsqrtf, inv_keep)"""
        return V(torch.tensor(float(x64), dtype=F64), torch.tensor(roundings * U * abs(float(x64)), dtype=F64)) if self.ref \
            else torch.tensor(float(x64), dtype=F64).float()

    def wr(self, hb, idx, val, valid=None):
        idx = torch.as_tensor(idx)
        if not isinstance(val, V) and not torch.is_tensor(val):
            val = torch.as_tensor(val, dtype=F32)
        val = val.expand(*idx.shape)
        if valid is not None:
            valid = valid.expand(*idx.shape)
            idx, val = idx[valid], val[valid]
        self.recs.append((hb, idx.reshape(-1), val.reshape(-1)))

    def seq_sum(self, terms, start=None):
        """a sum in the order given"""
        t = start
        for x in terms:
            t = x if t is None else t + x
        return t

    def any_sum(self, start, terms):
        """start + the terms [..., n] added in an order nobody fixes (fp32 atomics): n U (|start| + sum|terms|) on top of the terms'
        own bounds; the model adds them in index order"""
        if self.ref:
            n = terms.v.shape[-1]
            mag = start.v.abs() + start.e + (terms.v.abs() + terms.e).sum(-1)
            return V(start.v + terms.v.sum(-1), start.e + terms.e.sum(-1) + n * U * mag)
        t = start
        for k in range(terms.shape[-1]):
            t = t + terms[..., k]
        return t

    def zeros(self, *shape):
        return V(torch.zeros(*shape, dtype=F64)) if self.ref else torch.zeros(*shape)

    def set_err(self, val, err):
        """a bound derived by hand where the operands' errors are correlated and cancel (stated at the call)"""
        return V(val.v, err) if self.ref else val


class Case:
    def __init__(self, fam, name, bufs, kern, launch, exact=False, extra=None):
        self.fam, self.name, self.bufs, self.kern, self.launch, self.exact, self.extra = fam, name, bufs, kern, launch, exact, extra


def _within(fam, name, got, ref, allow):
    """every element of got within allow of ref (NaN anywhere fails); records the worst err / allowed of the family"""
    err = (got.double() - ref).abs()
    ok = err <= allow
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allow.clamp(min=1e-300)).nan_to_num(nan=float("inf"))
    w = float(ratio.max()) if ratio.numel() else 0.0
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError("%s: %d/%d outside the bound, first at %d: got %.9g, ref %.9g, allowed %.3g; worst err/allowed %.3g" % (
            name, int((~ok).sum()), ok.numel(), i, float(got[i]), float(ref[i]), float(allow[i]), w))
    WORST[fam] = max(WORST.get(fam, 0.0), w)
    return w


def _same_bits(name, got, ref):
    if not torch.equal(_bits(got), _bits(ref)):
        bad = (_bits(got) != _bits(ref)).nonzero()
        i = int(bad[0])
        raise AssertionError("%s: %d/%d elements differ in bits, first at %d: got %.9g, expected %.9g" % (
            name, len(bad), got.numel(), i, float(got[i]), float(ref[i])))


def _verify(case, after):
    """what was written against the restatement; everything else against the image the call started from"""
    ref = Ctx(True)
    case.kern(ref)
    m32 = None
    if case.exact:                                          # the float32 operation sequence: the bits an exact case must give
        m32 = Ctx(False)
        case.kern(m32)
    written = {k: torch.zeros(hb.host.numel(), dtype=torch.bool) for k, hb in case.bufs.items() if hb is not None}
    names = {id(hb): k for k, hb in case.bufs.items() if hb is not None}
    worst = 0.0
    for n, (hb, idx, val) in enumerate(ref.recs):
        k = names[id(hb)]
        pos = hb.base + idx
        assert int(pos.min()) >= PAD and int(pos.max()) < PAD + hb.n and not bool(written[k][pos].any()), case.name + ": the case's own indices"
        got = after[k][pos]
        lab = "%s %s" % (case.name, k)
        assert not bool(torch.isnan(val.v).any()), lab + ": the reference read a poisoned element"
        if case.exact:
            want = m32.recs[n][2].to(hb.dtype)
            if case.exact == "integer":                     # exact in any order: the float64 value itself, rounded once
                assert torch.equal(val.v.float().double(), val.v) and torch.equal(m32.recs[n][2].double(), val.v), lab + ": not an exact case"
            _same_bits(lab, got, want)
        else:
            e = val.e + (_half_ulp(val.v.abs() + val.e, BF) if hb.dtype == BF else 0.0)
            worst = max(worst, _within(case.fam + (" (bf16 store)" if hb.dtype == BF else ""), lab, got, val.v, e))
        written[k][pos] = True
    for k, hb in case.bufs.items():
        if hb is not None:
            keep = ~written[k]
            assert torch.equal(_bits(after[k][keep]), _bits(hb.host[keep])), "%s %s: %d elements outside the entry's output changed (pads, other steps, operands)" % (
                case.name, k, int((_bits(after[k][keep]) != _bits(hb.host[keep])).sum()))
    if case.extra:
        case.extra(after)
    return worst


def _model_run(case, defect=None):
    c = Ctx(False, defect)
    case.kern(c)
    after = {k: hb.host.clone() for k, hb in case.bufs.items() if hb is not None}
    names = {id(hb): k for k, hb in case.bufs.items() if hb is not None}
    for hb, idx, val in c.recs:
        pos = (hb.base + idx)
        ok = (pos >= 0) & (pos < hb.host.numel())
        after[names[id(hb)]][pos[ok]] = val[ok].to(hb.dtype)
    return after


def _gpu_run(case, launch=None):
    dev = {k: hb.host.to(DEV) for k, hb in case.bufs.items() if hb is not None}

    def p(k):
        return None if case.bufs.get(k) is None else dev[k][case.bufs[k].base:]
    (launch or case.launch)(p)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dev.items()}


def _run_cases(cases, model=False):
    for case in cases:
        _verify(case, _model_run(case) if model else _gpu_run(case))


def _rc(rc, what):
    assert rc == 0, "%s failed (%d): %s" % (what, rc, hip.lib().mmtg_last_error().decode())


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# =====================================================================================================================
# 1. recurrent cells
# =====================================================================================================================
CELL_SIZES = [(1, 8), (1, 256), (3, 100), (2, 129), (7, 512)]
CELL_FORMS = ["nat", "step", "gh0", "null"]


def _cell_index(c, B, H):
    n = B * H
    if c.defect == "tail":                                  # the workgroup that holds the B H tail does nothing
        n = n // 256 * 256
    i = _ar(n)
    return i, i // H, i % H


def k_gru_fwd(c, gi, gh, hp, h, save, B, H):
    i, b, j = _cell_index(c, B, H)
    ld_gi, ld_gh, ld_h = gi.ld, gh.ld, h.ld
    if c.defect == "natural_stride":
        ld_gi, ld_h = 3 * H, H
    if c.defect == "ld_gh":
        ld_gh = 3 * H
    o, oi = b * ld_gh + j, b * ld_gi + j
    r = fsig(c.rd(gi, oi) + c.rd(gh, o))
    z = fsig(c.rd(gi, oi + H) + c.rd(gh, o + H))
    ghn = c.rd(gh, o + 2 * H)
    n = ftanh(c.rd(gi, oi + 2 * H) + r * ghn)
    hv = (1.0 - z) * n
    if hp is not None:
        hv = hv + z * c.rd(hp, b * hp.ld + j)
    else:
        hv = hv + z * 0.0
    c.wr(h, b * ld_h + j, hv)
    BH = B * H
    for k, x in enumerate((r, z, n, ghn)):
        c.wr(save, k * BH + i, x)


def _gru_bwd_body(c, d, i, b, j, save, hp, dgi, dgh, dhp, B, H):
    BH = B * H
    R, Z = (0, 1) if c.defect != "rz_swap" else (1, 0)
    r, z, n, ghn = c.rd(save, R * BH + i), c.rd(save, Z * BH + i), c.rd(save, 2 * BH + i), c.rd(save, 3 * BH + i)
    hpv = c.rd(hp, b * hp.ld + j) if hp is not None else 0.0 * n
    dz = d * (hpv - n)
    dn = d * (1.0 - z)
    da = dn * (1.0 - n * n)
    dr = da * ghn
    dr_pre = dr * r * (1.0 - r)
    dz_pre = dz * z * (1.0 - z)
    o, oi = b * 3 * H + j, b * dgi.ld + j
    c.wr(dgi, oi, dr_pre), c.wr(dgi, oi + H, dz_pre), c.wr(dgi, oi + 2 * H, da)
    c.wr(dgh, o, dr_pre), c.wr(dgh, o + H, dz_pre), c.wr(dgh, o + 2 * H, da if c.defect == "dgh_r" else da * r)
    c.wr(dhp, i, d * z)


def k_gru_bwd(c, dh, save, hp, dgi, dgh, dhp, B, H):
    i, b, j = _cell_index(c, B, H)
    _gru_bwd_body(c, c.rd(dh, i), i, b, j, save, hp, dgi, dgh, dhp, B, H)


def k_gru_fused(c, rows, carry, part, splits, save, hp, dgi, dgh, dhp, B, H):
    i, b, j = _cell_index(c, B, H)
    d = c.rd(rows, b * rows.ld + j)
    if carry is not None:
        d = d + c.rd(carry, i)
        if c.defect == "carry_twice":
            d = d + c.rd(carry, i)
    for k in range(splits - 1 if c.defect == "last_slab" else splits):
        d = d + c.rd(part, k * B * H + i)
    _gru_bwd_body(c, d, i, b, j, save, hp, dgi, dgh, dhp, B, H)


def k_rnn_fwd(c, kind, gi, gh, cp, h, cc, save, B, H):
    i, b, j = _cell_index(c, B, H)
    o, oi = b * gh.ld + j, b * gi.ld + j
    if kind == 0:
        c.wr(h, b * h.ld + j, frelu(c.rd(gi, oi) + c.rd(gh, o)))
        return
    gi_ = fsig(c.rd(gi, oi) + c.rd(gh, o))
    gf = fsig(c.rd(gi, oi + H) + c.rd(gh, o + H))
    gg = ftanh(c.rd(gi, oi + 2 * H) + c.rd(gh, o + 2 * H))
    go = fsig(c.rd(gi, oi + 3 * H) + c.rd(gh, o + 3 * H))
    cn = gf * (c.rd(cp, i) if cp is not None else 0.0) + gi_ * gg
    tc = ftanh(cn)
    c.wr(cc, i, cn)
    c.wr(h, b * h.ld + j, go * tc)
    for k, x in enumerate((gi_, gf, gg, go, tc)):
        c.wr(save, k * B * H + i, x)


def k_rnn_bwd(c, kind, rows, part, save, cp, h, dc, dc_in, da, B, H):
    i, b, j = _cell_index(c, B, H)
    d = c.rd(rows, b * rows.ld + j)
    if part is not None:
        d = d + c.rd(part, i)
    oa = b * da.ld + j
    if kind == 0:
        c.wr(da, oa, fwhere(c.ids(h, b * h.ld + j).float() > 0, d, c.zeros(*i.shape)))
        return
    BH = B * H
    gi_, gf, gg, go, tc = (c.rd(save, k * BH + i) for k in range(5))
    t = d * go * (1.0 - tc * tc)
    dct = (c.rd(dc, i) + t) if (dc_in and c.defect != "dc_in") else (0.0 + t)
    cpv = c.rd(cp, i) if cp is not None else 0.0 * gf
    c.wr(da, oa, dct * gg * gi_ * (1.0 - gi_))
    c.wr(da, oa + H, dct * cpv * gf * (1.0 - gf))
    c.wr(da, oa + 2 * H, dct * gi_ * (1.0 - gg * gg))
    c.wr(da, oa + 3 * H, d * tc * go * (1.0 - go))
    c.wr(dc, i, dct * gf)


def _preact(B, W, seed, data, G_):
    """pre-activation halves gi, gh [B, W]: random with |gi + gh| <= ARG_MAX; saturated: gi = +-100 alternating by (column + block),
    gh = 0; zeros (the ReLU cell): a exactly -0.0, +0 (1 - 1), a small negative and a small positive"""
    if data == "saturated":
        col = _ar(W)
        sg = 1.0 - 2.0 * (((col % (W // G_)) + col // (W // G_) + _ar(B)[:, None]) % 2).float()
        return 100.0 * sg, torch.zeros(B, W)
    if data == "zeros":
        k = (_ar(W)[None, :] + _ar(B)[:, None]) % 4
        gi = torch.tensor([-0.0, 1.0, -0.25, 0.5])[k]
        gh = torch.tensor([-0.0, -1.0, 0.125, -0.25])[k]
        return gi, gh
    return _randn(B, W, seed=seed, scale=4.0).clamp(-ARG_MAX / 2, ARG_MAX / 2), _randn(B, W, seed=seed + 1, scale=2.0).clamp(-2.0, 2.0)


def _stp(form):
    return (3, 1) if form == "step" else (1, 0)


def gru_fwd_case(bf, B, H, form, data="random"):
    T, (S, t) = _T(bf), _stp(form)
    gi_, gh_ = _preact(B, 3 * H, 11 * H + B, data, 3)
    gi = _rows(B, 3 * H, T, gi_, S, t)
    gh = _rows(1, 3 * H, T, gh_[:1]) if form == "gh0" else _rows(B, 3 * H, T, gh_)
    if form == "gh0":
        gh.ld = 0
    hp = None if form == "null" else _rows(B, H, T, _randn(B, H, seed=7 * H + B), S, t)
    h, save = _rows(B, H, T, None, S, t), _outv(4 * B * H)
    bufs = dict(gi=gi, gh=gh, hp=hp, h=h, save=save)

    def launch(p):
        hip.gru_cell_fwd(p("gi"), p("gh"), p("hp"), p("h"), p("save"), B, H, ld_gi=gi.ld, ld_hp=hp.ld if hp else H, ld_h=h.ld, ld_gh=gh.ld)
    return Case("gru_cell_fwd", "gru_fwd %s B=%d H=%d %s %s" % (T, B, H, form, data), bufs,
                lambda c: k_gru_fwd(c, gi, gh, hp, h, save, B, H), launch)


def _gru_save(B, H, exact):
    if exact:                # dyadic planes: every product of the backward has at most 16 significant bits
        return torch.cat([_pick([0.25, 0.5, 0.75], B * H, seed=3 * H + B), _pick([0.25, 0.5, 0.75], B * H, seed=3 * H + B + 1),
                          _pick([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75], B * H, seed=3 * H + B + 2),
                          _pick([-2.0, -1.5, -0.5, 0.0, 0.5, 1.0, 2.0], B * H, seed=3 * H + B + 3)])
    g = _gen(5 * H + B)
    return torch.cat([torch.rand(2 * B * H, generator=g) * 0.98 + 0.01, torch.rand(B * H, generator=g) * 1.96 - 0.98,
                      torch.randn(B * H, generator=g)])


def _hprev(B, H, exact, seed):
    return _pick([-2.0, -1.25, -0.5, 0.0, 0.25, 1.0, 1.75], B, H, seed=seed) if exact else _randn(B, H, seed=seed)


def gru_bwd_case(bf, B, H, form, exact, fused=None):
    """fused: None (mmtg_gru_cell_bwd) or (splits, carry) with carry in (None, "own", "alias")"""
    T, (S, t) = _T(bf), _stp(form)
    save = _vec(_gru_save(B, H, exact))
    hp = None if form == "null" else _rows(B, H, T, _hprev(B, H, exact, 9 * H + B), S, t)
    dgi, dgh, dhp = _rows(B, 3 * H, T, None, S, t), _rows(B, 3 * H, T, None), _outv(B * H)
    dsrc = _ints(-4, 4, B, H, seed=13 * H + B) if exact else _randn(B, H, seed=13 * H + B)
    ldhp = hp.ld if hp else H
    if fused is None:
        dh = _vec(dsrc)
        bufs = dict(dh=dh, save=save, hp=hp, dgi=dgi, dgh=dgh, dhp=dhp)

        def launch(p):
            hip.gru_cell_bwd(p("dh"), p("save"), p("hp"), p("dgi"), p("dgh"), p("dhp"), B, H, ld_hp=ldhp, ld_dgi=dgi.ld)
        return Case("gru_cell_bwd", "gru_bwd %s B=%d H=%d %s %s" % (T, B, H, form, "exact" if exact else "random"), bufs,
                    lambda c: k_gru_bwd(c, dh, save, hp, dgi, dgh, dhp, B, H), launch, exact="integer" if exact else False)
    splits, cmode = fused
    rows = _rows(B, H, T, dsrc, S, t)
    mk = (lambda s: _ints(-3, 3, B * H, seed=s)) if exact else (lambda s: _randn(B * H, seed=s))
    part = _vec(torch.cat([mk(17 * H + B + k) for k in range(splits)])) if splits else None
    carry = None
    if cmode == "own":
        carry = _vec(mk(19 * H + B))
    elif cmode == "alias":                                   # the engine's use: dh_prev holds the carry on entry
        dhp = carry = _acc(mk(19 * H + B))
    bufs = dict(rows=rows, part=part, save=save, hp=hp, dgi=dgi, dgh=dgh, dhp=dhp)
    if cmode == "own":
        bufs["carry"] = carry

    def launch(p):
        hip.gru_cell_bwd_fused(p("rows"), rows.ld, p("dhp") if cmode == "alias" else p("carry"), p("part"), splits, p("save"), p("hp"),
                               p("dgi"), p("dgh"), p("dhp"), B, H, ld_hp=ldhp, ld_dgi=dgi.ld)
    return Case("gru_cell_bwd_fused", "gru_fused %s B=%d H=%d %s %s splits=%d carry=%s" % (T, B, H, form, "exact" if exact else "random", splits, cmode),
                bufs, lambda c: k_gru_fused(c, rows, carry, part, splits, save, hp, dgi, dgh, dhp, B, H), launch, exact="integer" if exact else False)


def rnn_fwd_case(bf, kind, B, H, form, data="random"):
    T, (S, t), G_ = _T(bf), _stp(form), 4 if kind else 1
    gi_, gh_ = _preact(B, G_ * H, 23 * H + B + kind, data, G_)
    gi = _rows(B, G_ * H, T, gi_, S, t)
    gh = _rows(1, G_ * H, T, gh_[:1]) if form == "gh0" else _rows(B, G_ * H, T, gh_)
    if form == "gh0":
        gh.ld = 0
    cp = _vec(_randn(B * H, seed=29 * H + B)) if kind and form != "null" else None
    h = _rows(B, H, T, None, S, t)
    cc, save = (_outv(B * H), _outv(5 * B * H)) if kind else (None, None)
    bufs = dict(gi=gi, gh=gh, cp=cp, h=h, c=cc, save=save)

    def launch(p):
        hip.rnn_cell_fwd(kind, p("gi"), p("gh"), p("cp"), p("h"), p("c"), p("save"), B, H, gi.ld, h.ld, ld_gh=gh.ld)
    return Case("rnn_cell_fwd " + ("lstm" if kind else "relu"), "rnn_fwd kind=%d %s B=%d H=%d %s %s" % (kind, T, B, H, form, data), bufs,
                lambda c: k_rnn_fwd(c, kind, gi, gh, cp, h, cc, save, B, H), launch)


def rnn_bwd_case(bf, kind, B, H, form, exact, dc_in=0):
    T, (S, t), G_ = _T(bf), _stp(form), 4 if kind else 1
    rows = _rows(B, H, T, _ints(-4, 4, B, H, seed=31 * H + B) if exact else _randn(B, H, seed=31 * H + B), S, t)
    part = None if form == "null" else _vec(_ints(-3, 3, B * H, seed=37 * H + B) if exact else _randn(B * H, seed=37 * H + B))
    da = _rows(B, G_ * H, T, None, S, t)
    save = cp = h = dc = None
    if kind:
        if exact:
            pl = [_pick([0.25, 0.5, 0.75], B * H, seed=41 * H + B + k) for k in (0, 1)] + [_pick([-0.75, -0.25, 0.0, 0.5], B * H, seed=41 * H + B + 2),
                  _pick([0.25, 0.5, 0.75], B * H, seed=41 * H + B + 3), _pick([-0.75, -0.5, 0.0, 0.25, 0.75], B * H, seed=41 * H + B + 4)]
        else:
            g = _gen(43 * H + B)
            u = lambda: torch.rand(B * H, generator=g)      # noqa: E731
            pl = [u() * 0.98 + 0.01, u() * 0.98 + 0.01, u() * 1.96 - 0.98, u() * 0.98 + 0.01, u() * 1.96 - 0.98]
        save = _vec(torch.cat(pl))
        cp = None if form == "null" else _vec(_hprev(1, B * H, exact, 47 * H + B))
        dc = _acc(_ints(-3, 3, B * H, seed=53 * H + B) if exact else _randn(B * H, seed=53 * H + B)) if dc_in else _outv(B * H)
    else:                    # the stored output of the ReLU cell: zeros (exactly 0 and -0.0) and positives
        hv = _pick([0.0, -0.0, 0.5, 2.0, 0.0078125], B, H, seed=59 * H + B)
        h = _rows(B, H, T, hv, S, t)
    bufs = dict(rows=rows, part=part, save=save, cp=cp, h=h, dc=dc, da=da)

    def launch(p):
        hip.rnn_cell_bwd(kind, p("rows"), rows.ld, p("part"), p("save"), p("cp"), p("h"), h.ld if h else H, p("dc"), dc_in, p("da"), da.ld, B, H)
    return Case("rnn_cell_bwd " + ("lstm" if kind else "relu"), "rnn_bwd kind=%d %s B=%d H=%d %s %s dc_in=%d" % (kind, T, B, H, form, "exact" if exact else "random", dc_in),
                bufs, lambda c: k_rnn_bwd(c, kind, rows, part, save, cp, h, dc, dc_in, da, B, H), launch, exact="integer" if exact else False)


def cell_cases(entry, bf):
    """every size in every form for the forward; the backward in the forms it has (no ld_gh)"""
    out = []
    for B, H in CELL_SIZES:
        for form in CELL_FORMS:
            if entry == "gru_fwd":
                out.append(gru_fwd_case(bf, B, H, form))
                if form in ("nat", "step"):
                    out.append(gru_fwd_case(bf, B, H, form, "saturated"))
            elif entry in ("lstm_fwd", "relu_fwd"):
                kind = int(entry == "lstm_fwd")
                out.append(rnn_fwd_case(bf, kind, B, H, form))
                if form in ("nat", "step"):
                    out.append(rnn_fwd_case(bf, kind, B, H, form, "saturated"))
                    if not kind:
                        out.append(rnn_fwd_case(bf, kind, B, H, form, "zeros"))
            elif form != "gh0":
                for exact in (True, False):
                    if entry == "gru_bwd":
                        out.append(gru_bwd_case(bf, B, H, form, exact))
                    elif entry == "gru_fused":
                        for fused in ((0, None), (0, "alias"), (1, "own"), (3, "alias"), (3, None)):
                            out.append(gru_bwd_case(bf, B, H, form, exact, fused))
                    elif entry == "lstm_bwd":
                        out.append(rnn_bwd_case(bf, 1, B, H, form, exact, 0))
                        out.append(rnn_bwd_case(bf, 1, B, H, form, exact, 1))
                    elif entry == "relu_bwd":
                        out.append(rnn_bwd_case(bf, 0, B, H, form, exact))
    return out


CELL_ENTRIES = ["gru_fwd", "gru_bwd", "gru_fused", "lstm_fwd", "relu_fwd", "lstm_bwd", "relu_bwd"]


# =====================================================================================================================
# 2. alpha attention
# =====================================================================================================================
def _alpha_geom(c, B, H, heads):
    dh = H // heads
    b, hd, lane = _ar(B)[:, None, None], _ar(heads)[None, :, None], _ar(64)[None, None, :]
    hoff = hd * (dh if c.defect != "head_offset" else 0)
    lim = dh if (c.defect != "lane_tail" or dh < 64) else dh // 64 * 64
    chunks = [(lane + 64 * n, ((lane + 64 * n) < lim).expand(B, heads, 64)) for n in range(_cdiv(dh, 64))]
    return dh, b, hd, hoff, chunks


def k_alpha_fwd(c, qkv, prior, ctx, probs, kl, B, S, H, heads):
    dh, b, hd, hoff, chunks = _alpha_geom(c, B, H, heads)
    scale = c.const(1.0 / math.sqrt(dh), 2)
    ld = lambda i, blk, cc, ok: c.rd(qkv, (b * S + i) * 3 * H + blk * H + hoff + cc, ok)     # noqa: E731
    q = [[ld(i, 0, cc, ok) for cc, ok in chunks] for i in range(S)]
    k = [[ld(i, 1, cc, ok) for cc, ok in chunks] for i in range(S)]
    v = [[ld(i, 2, cc, ok) for cc, ok in chunks] for i in range(S)]
    sc = [[None] * S for _ in range(S)]
    for i in range(S):
        for j in range(S):
            a = wave_sum(c.seq_sum([q[i][n] * k[j][n] for n in range(len(chunks))]))
            sc[i][j] = a if c.defect == "alpha_scale" else a * scale
    klacc = None
    for i in range(S):
        mx = fshift(sc[i])
        e = [fexp(sc[i][j] - mx) for j in range(S)]
        inv = 1.0 / c.seq_sum(e)
        for j in range(S):
            sc[i][j] = e[j] * inv
            qp = c.rd(prior, torch.tensor(i * S + j))
            term = qp * (flog(qp) - flog(sc[i][j]))
            klacc = term if klacc is None else klacc + term
    pb = (b * heads + hd)[..., 0]
    for i in range(S):
        for j in range(S):
            c.wr(probs, (pb * S + i) * S + j, sc[i][j])
    terms = klacc / c.const(float(B) * S, 0)
    c.wr(kl, torch.tensor([0]), c.any_sum(c.rd(kl, torch.tensor([0])), terms.reshape(-1)))
    for n, (cc, ok) in enumerate(chunks):
        for i in range(S):
            a = c.seq_sum([sc[i][j][..., None] * v[j][n] for j in range(S)])
            c.wr(ctx, (b * S + i) * H + hoff + cc, a, ok)


def k_alpha_bwd(c, qkv, prior, probs, dctx, dkl, dqkv, B, S, H, heads):
    dh, b, hd, hoff, chunks = _alpha_geom(c, B, H, heads)
    scale = c.const(1.0 / math.sqrt(dh), 2)
    pb = (b * heads + hd)[..., 0]
    ld = lambda i, blk, cc, ok: c.rd(qkv, (b * S + i) * 3 * H + blk * H + hoff + cc, ok)     # noqa: E731
    q = [[ld(i, 0, cc, ok) for cc, ok in chunks] for i in range(S)]
    k = [[ld(i, 1, cc, ok) for cc, ok in chunks] for i in range(S)]
    v = [[ld(i, 2, cc, ok) for cc, ok in chunks] for i in range(S)]
    dc = [[c.rd(dctx, (b * S + i) * H + hoff + cc, ok) for cc, ok in chunks] for i in range(S)]
    P = [[c.rd(probs, (pb * S + i) * S + j) for j in range(S)] for i in range(S)]
    dklc = c.const(float(np.float32(dkl)), 0)
    dS = [[None] * S for _ in range(S)]
    for i in range(S):
        for j in range(S):
            a = wave_sum(c.seq_sum([dc[i][n] * v[j][n] for n in range(len(chunks))]))
            dS[i][j] = a - dklc * c.rd(prior, torch.tensor(i * S + j)) / (P[i][j] * float(B) * float(S))
    for i in range(S):
        dot = c.seq_sum([P[i][j] * dS[i][j] for j in range(S)])
        for j in range(S):
            dS[i][j] = P[i][j] * (dS[i][j] - dot) * scale
    for n, (cc, ok) in enumerate(chunks):
        for i in range(S):
            dq = c.seq_sum([dS[i][j][..., None] * k[j][n] for j in range(S)])
            dk = c.seq_sum([(dS[i][j] if c.defect == "dk_transposed" else dS[j][i])[..., None] * q[j][n] for j in range(S)])
            dv = c.seq_sum([P[j][i][..., None] * dc[j][n] for j in range(S)])
            o = (b * S + i) * 3 * H + hoff + cc
            c.wr(dqkv, o, dq, ok), c.wr(dqkv, o + H, dk, ok), c.wr(dqkv, o + 2 * H, dv, ok)


def _prior(S, seed):
    p = torch.rand(S, S, generator=_gen(seed)) + 0.1
    return (p / p.sum(-1, keepdim=True)).float()


def _alpha_qkv(bf, B, S, H, heads, data):
    """[B, S, 3 H].  random: asymmetric q and k of different spread.  exact: q = 0, so that every score is equal, and integer v: probs
    exactly 1 / S (S a power of two) and ctx the exact mean.  peaked: q and k large multiples of a shared direction per step, score
    gaps up to about 40"""
    dh = H // heads
    x = _randn(B, S, 3 * H, seed=100 * S + H + heads + B)
    if data == "random":
        x[..., :H] *= 1.5
        x[..., H:2 * H] = x[..., H:2 * H] * 0.7 + 0.3
    elif data == "exact":
        x[..., :H] = 0.0
        x[..., 2 * H:] = 8.0 * _ints(-4, 4, B, S, H, seed=7 * S + H)
    elif data == "peaked":
        u = torch.ones(H) / math.sqrt(dh)
        lev = torch.linspace(0.0, 1.0, S)[None, :, None]
        x[..., :H] = math.sqrt(40.0) * dh ** 0.25 * u + 0.05 * x[..., :H]
        x[..., H:2 * H] = math.sqrt(40.0) * dh ** 0.25 * u * lev + 0.05 * x[..., H:2 * H]
    return x.to(_T(bf))


def alpha_fwd_case(bf, B, S, H, heads, data="random"):
    T = _T(bf)
    qkv = _rows(B * S, 3 * H, T, _alpha_qkv(bf, B, S, H, heads, data))
    prior = _vec(torch.ones(1, 1) if S == 1 else _prior(S, S))
    ctx, probs, kl = _rows(B * S, H, T, None), _outv(B * heads * S * S), _acc(torch.tensor([3.0]))
    bufs = dict(qkv=qkv, prior=prior, ctx=ctx, probs=probs, kl=kl)

    def launch(p):
        hip.alpha_attn_fwd(p("qkv"), p("prior"), p("ctx"), p("probs"), p("kl"), B, S, H, heads)

    def extra(after):
        pr = after["probs"][PAD:PAD + probs.n]
        if S == 1:           # probs exactly 1, kl unchanged, ctx equal to v bit for bit
            assert bool((pr == 1.0).all()) and float(after["kl"][PAD]) == 3.0
            _same_bits("ctx = v", after["ctx"][PAD:PAD + ctx.n].view(B, H), qkv.host[PAD:PAD + qkv.n].view(B, 3 * H)[:, 2 * H:])
        if data == "exact" and S in (2, 4, 8):
            assert bool((pr == 1.0 / S).all()), "probs must be exactly 1 / S"
            vm = qkv.host[PAD:PAD + qkv.n].view(B, S, 3 * H)[..., 2 * H:].double().mean(1, keepdim=True).expand(B, S, H)
            _same_bits("ctx = mean v", after["ctx"][PAD:PAD + ctx.n].view(B, S, H), vm.float().to(T))
    name = "alpha_fwd %s B=%d S=%d H=%d heads=%d %s" % (T, B, S, H, heads, data)
    return Case("alpha_attn_fwd", name, bufs, lambda c: k_alpha_fwd(c, qkv, prior, ctx, probs, kl, B, S, H, heads), launch, extra=extra)


def alpha_bwd_case(bf, B, S, H, heads, data, dkl, probs_data):
    """probs_data: the probs a forward run stored ([B heads S S] fp32)"""
    T = _T(bf)
    qkv = _rows(B * S, 3 * H, T, _alpha_qkv(bf, B, S, H, heads, data))
    prior = _vec(torch.ones(1, 1) if S == 1 else _prior(S, S))
    probs = _vec(probs_data)
    dctx = _rows(B * S, H, T, _randn(B * S, H, seed=300 * S + H + B) + 0.25)
    dqkv = _rows(B * S, 3 * H, T, None)
    bufs = dict(qkv=qkv, prior=prior, probs=probs, dctx=dctx, dqkv=dqkv)

    def launch(p):
        hip.alpha_attn_bwd(p("qkv"), p("prior"), p("probs"), p("dctx"), dkl, p("dqkv"), B, S, H, heads)
    name = "alpha_bwd %s B=%d S=%d H=%d heads=%d %s dkl=%g" % (T, B, S, H, heads, data, dkl)
    return Case("alpha_attn_bwd", name, bufs, lambda c: k_alpha_bwd(c, qkv, prior, probs, dctx, dkl, dqkv, B, S, H, heads), launch)


# (B, S, H, heads): every S with one head of 64; every head width; one head and several with B = 1 and 3
ALPHA_SHAPES = [(1, s, 64, 1) for s in range(1, 9)] + [(1, 3, 8, 1), (3, 2, 16, 2), (1, 5, 72, 1), (3, 8, 288, 4), (1, 4, 128, 1),
                (3, 5, 512, 4), (1, 8, 256, 1), (3, 2, 512, 2), (1, 7, 320, 1), (3, 3, 640, 2), (1, 6, 512, 4), (3, 1, 144, 2)]
ALPHA_SPECIAL = [(2, s, 144, 2, "exact") for s in (2, 4, 8)] + [(3, 1, 64, 1, "exact"), (2, 5, 144, 2, "peaked"), (1, 8, 320, 1, "peaked"), (3, 3, 16, 2, "peaked")]


def alpha_cases():
    return [(B, S, H, hd, "random") for B, S, H, hd in ALPHA_SHAPES] + ALPHA_SPECIAL


def _alpha_pair(bf, shape, run):
    """forward, then the backward on the probs that forward stored, dkl 0 and 0.37 (the peaked case: 0 only -- prior / P has no bound)"""
    B, S, H, heads, data = shape
    fw = alpha_fwd_case(bf, B, S, H, heads, data)
    if data == "peaked":     # the condition on the case itself: its smallest float64 probability stays representable
        r = Ctx(True)
        fw.kern(r)
        pmin = min(float(val.v.min()) for hb, idx, val in r.recs if hb is fw.bufs["probs"])
        assert 1e-30 < pmin < 1e-12, pmin
    after = run(fw)
    _verify(fw, after)
    stored = after["probs"][PAD:PAD + fw.bufs["probs"].n].clone()
    for dkl in ((0.0,) if data == "peaked" else (0.0, 0.37)):
        bw = alpha_bwd_case(bf, B, S, H, heads, data, dkl, stored)
        _verify(bw, run(bw))


# =====================================================================================================================
# 3. beta fuser
# =====================================================================================================================
def _beta_geom(c, B, S, H):
    b, i, lane = _ar(B)[:, None, None], _ar(S)[None, :, None], _ar(64)[None, None, :]
    chunks = [(lane + 64 * n, ((lane + 64 * n) < H).expand(B, S, 64)) for n in range(_cdiv(H, 64))]
    return b, i, b * S + i, chunks


def k_beta_fwd(c, topic, img, txt, att_w, att_b, o, a_out, B, S, H):
    b, i, r, chunks = _beta_geom(c, B, S, H)
    tv = [c.rd(topic, b * H + cc + 0 * i, ok) for cc, ok in chunks]
    iv = [c.rd(img, r * H + cc, ok) for cc, ok in chunks]
    xv = [c.rd(txt, r * H + cc, ok) for cc, ok in chunks]
    w = [c.rd(att_w, i * H + cc + 0 * b, ok) for cc, ok in chunks]
    bb = c.rd(att_b, (i + 0 * b)[..., 0])
    s = [wave_sum(c.seq_sum([w[n] * x[n] for n in range(len(chunks))])) for x in (tv, iv, xv)]
    # (the bias is the same on all three scores and cancels in the softmax: leaving it out altogether changes no output, so the
    #  planted defect leaves it out of the image and text scores only)
    s = [s[0] + bb] + [sk if c.defect == "fuser_bias" else sk + bb for sk in s[1:]]
    mx = fshift(s)
    e = [fexp(sk - mx) for sk in s]
    inv = 1.0 / (e[0] + e[1] + e[2])
    e = [ek * inv for ek in e]
    for n, (cc, ok) in enumerate(chunks):
        c.wr(o, r * H + cc, e[0][..., None] * tv[n] + e[1][..., None] * iv[n] + e[2][..., None] * xv[n], ok)
    for k in range(3):
        c.wr(a_out, r[..., 0] * 3 + k, e[k])


def k_beta_bwd(c, topic, img, txt, att_w, a_in, d_o, dtopic, dimg, dtxt, datt_w, datt_b, B, S, H, atomic):
    b, i, r, chunks = _beta_geom(c, B, S, H)
    a = [c.rd(a_in, r[..., 0] * 3 + k) for k in range(3)]
    tv = [c.rd(topic, b * H + cc + 0 * i, ok) for cc, ok in chunks]
    iv = [c.rd(img, r * H + cc, ok) for cc, ok in chunks]
    xv = [c.rd(txt, r * H + cc, ok) for cc, ok in chunks]
    dv = [c.rd(d_o, r * H + cc, ok) for cc, ok in chunks]
    d = [wave_sum(c.seq_sum([dv[n] * x[n] for n in range(len(chunks))])) for x in (tv, iv, xv)]
    ad = [a[k] * d[k] for k in range(3)]
    dot = ad[0] + ad[1] + ad[2]
    ds = [a[k] * (d[k] - dot) for k in range(3)]
    for n, (cc, ok) in enumerate(chunks):
        w = c.rd(att_w, i * H + cc + 0 * b, ok)
        gt = a[0][..., None] * dv[n] + ds[0][..., None] * w
        gw = ds[0][..., None] * tv[n] + ds[1][..., None] * iv[n] + ds[2][..., None] * xv[n]
        c.wr(dimg, r * H + cc, a[1][..., None] * dv[n] + ds[1][..., None] * w, ok)
        c.wr(dtxt, r * H + cc, a[2][..., None] * dv[n] + ds[2][..., None] * w, ok)
        ti, wi = (b * H + cc)[:, 0], (i * H + cc)[0]        # [B, 64], [S, 64]
        old_t, old_w = c.rd(dtopic, ti, ok[:, 0]), c.rd(datt_w, wi, ok[0])
        if c.defect == "dtopic_overwritten":
            old_t = 0.0 * old_t
        if atomic:
            c.wr(dtopic, ti, c.any_sum(old_t, _perm(gt, (0, 2, 1))), ok[:, 0])
        else:                # the steps in order through LDS, then one add onto what dtopic holds
            c.wr(dtopic, ti, old_t + c.seq_sum([gt[:, k] for k in range(S)]), ok[:, 0])
        c.wr(datt_w, wi, c.any_sum(old_w, _perm(gw, (1, 2, 0))), ok[0])
    # d att_b: ds0 + ds1 + ds2 = sum a_k d_k - dot sum a_k.  The computed d_k enter both halves and cancel whatever error they
    # carry; what is left is the rounding of dot (three products, two additions: 5 U sum|a_k d_k|), of each ds_k (a subtraction and
    # a product: 2 U |ds_k|) and of the two additions (2 U sum|ds_k|) -- U (5 sum|a_k d_k| + 4 sum|ds_k|) per (b, step) -- then the
    # sum over b.  The float64 value is dot (1 - sum a_k) on the stored weights, not zero.
    sb = ds[0] + ds[1] + ds[2]
    if c.ref:
        sb = c.set_err(sb, U * (5 * sum(x.v.abs() for x in ad) + 4 * sum(x.v.abs() for x in ds)) * (1 + 2.0 ** -10))
    old_b = c.rd(datt_b, _ar(S))
    c.wr(datt_b, _ar(S), c.any_sum(old_b, _perm(sb, (1, 0))))


def _perm(x, dims):
    return V(x.v.permute(*dims), x.e.permute(*dims)) if isinstance(x, V) else x.permute(*dims)


def _beta_operands(bf, B, S, H, integer):
    T, s = _T(bf), 1000 * H + 10 * S + B
    if integer:
        mk = lambda k, *sh: _ints(-3, 3, *sh, seed=s + k)   # noqa: E731
    else:
        mk = lambda k, *sh: _randn(*sh, seed=s + k)         # noqa: E731
    topic, img, txt = _rows(B, H, T, mk(0, B, H)), _rows(B * S, H, T, mk(1, B * S, H) + (0 if integer else 0.2)), _rows(B * S, H, T, mk(2, B * S, H))
    att_w = _vec(mk(3, S * H) if integer else mk(3, S * H) / math.sqrt(H))
    return T, topic, img, txt, att_w, mk


def beta_fwd_case(bf, B, S, H):
    T, topic, img, txt, att_w, mk = _beta_operands(bf, B, S, H, False)
    att_b = _vec(_randn(S, seed=H + S) + 1.0)
    o, a = _rows(B * S, H, T, None), _outv(B * S * 3)
    bufs = dict(topic=topic, img=img, txt=txt, att_w=att_w, att_b=att_b, o=o, a=a)

    def launch(p):
        hip.beta_fuse_fwd(p("topic"), p("img"), p("txt"), p("att_w"), p("att_b"), p("o"), p("a"), B, S, H)

    def extra(after):        # each weight is e_k inv: two roundings of the sum e0 + e1 + e2, one of 1 / sum, one of the product
        sm = after["a"][PAD:PAD + a.n].double().view(B * S, 3).sum(-1)
        assert bool(((sm - 1.0).abs() <= 4 * U * (1 + 2.0 ** -10)).all()), float((sm - 1.0).abs().max())
    return Case("beta_fuse_fwd", "beta_fwd %s B=%d S=%d H=%d" % (T, B, S, H), bufs,
                lambda c: k_beta_fwd(c, topic, img, txt, att_w, att_b, o, a, B, S, H), launch, extra=extra)


def beta_bwd_case(bf, B, S, H, atomic, integer=False):
    T, topic, img, txt, att_w, mk = _beta_operands(bf, B, S, H, integer)
    if integer:              # weights 1/2, 1/4, 1/4: every product and sum of the backward is a small dyadic number
        av = torch.tensor([0.5, 0.25, 0.25]).repeat(B * S)
    else:
        e = torch.rand(B * S, 3, generator=_gen(H + S + B)) + 0.05
        av = (e / e.sum(-1, keepdim=True)).float().reshape(-1)
    a = _vec(av)
    d_o = _rows(B * S, H, T, mk(5, B * S, H))
    dtopic, datt_w, datt_b = _acc(_ints(-3, 3, B * H, seed=1)), _acc(_ints(-3, 3, S * H, seed=2)), _acc(_ints(-3, 3, S, seed=3))
    dimg, dtxt = _rows(B * S, H, T, None), _rows(B * S, H, T, None)
    bufs = dict(topic=topic, img=img, txt=txt, att_w=att_w, a=a, d_o=d_o, dtopic=dtopic, dimg=dimg, dtxt=dtxt, datt_w=datt_w, datt_b=datt_b)

    def launch(p):
        if atomic:
            _rc(hip.lib().mmtg_beta_fuse_bwd(hip.dt(p("topic")), *[_ptr(p(k)) for k in ("topic", "img", "txt", "att_w", "a", "d_o", "dtopic", "dimg", "dtxt", "datt_w", "datt_b")],
                                             B, S, H, 0, 0, _stream()), "beta_fuse_bwd (atomic form)")
        else:
            hip.beta_fuse_bwd(*[p(k) for k in ("topic", "img", "txt", "att_w", "a", "d_o", "dtopic", "dimg", "dtxt", "datt_w", "datt_b")], B, S, H)
    name = "beta_bwd %s B=%d S=%d H=%d %s%s" % (T, B, S, H, "atomic" if atomic else "workspace", " integer" if integer else "")
    return Case("beta_fuse_bwd " + ("atomic" if atomic else "workspace"), name, bufs,
                lambda c: k_beta_bwd(c, topic, img, txt, att_w, a, d_o, dtopic, dimg, dtxt, datt_w, datt_b, B, S, H, atomic), launch,
                exact="integer" if integer else False)


# (B, S, H): every H, S and B of the issue once at least; (2, 16, 1024) is the 1024-thread, 64 KiB corner of the workspace form
BETA_SHAPES = [(1, 1, 8), (2, 2, 64), (9, 5, 100), (1, 16, 512), (2, 5, 1024), (9, 2, 8), (2, 16, 1024), (1, 5, 64)]


# =====================================================================================================================
# 4. embedding front end
# =====================================================================================================================
def _keep(seed, idx, p):
    """common.h dropout_scale restated: keep iff hash_u32(seed, idx) >= p 2^32"""
    thresh = hip.drop_thresh(p)
    if not thresh:
        return torch.ones(idx.shape, dtype=torch.bool), 1.0
    keep = _hash_u32(np.uint32(seed), (idx.numpy() & 0xFFFFFFFF).astype(np.uint32)) >= np.uint32(thresh)
    return torch.from_numpy(keep), 4294967296.0 / (4294967296.0 - float(thresh))


def k_embed_condition(c, table, topic_ids, targets, cvec, x, B, P, L, S, E, two_sents, Vn):
    Tt = P + L
    row = _ar(B * Tt)
    b, t = row // Tt, row % Tt
    p = (t - P).clamp(min=0)
    idt = c.ids(topic_ids, b * P + t.clamp(max=max(P - 1, 0))) if P else torch.zeros_like(row)
    ids = torch.where(t < P, idt, c.ids(targets, b * L + p))
    k = (p + 1) // two_sents if c.defect == "segment_edge" else p // two_sents
    seg = torch.where((t >= P) & (k < S), k, torch.full_like(k, -1))
    if c.defect != "id_clamp":
        ids = ids.clamp(0, Vn - 1)
    e = _ar(E)[None, :]
    v = c.rd(table, ids[:, None] * E + e)
    has = (seg >= 0)[:, None].expand(B * Tt, E)
    v = fwhere(has, v + c.rd(cvec, ((b * S + seg.clamp(min=0)) * E)[:, None] + e), v)
    c.wr(x, row[:, None] * E + e, v)


def k_segment_sum(c, g, out, B, P, L, S, H, two_sents):
    Tt = P + L
    b, h = _ar(B)[:, None], _ar(H)[None, :]
    for k in range(S):
        p0 = k * two_sents
        p1 = min(L, p0 + two_sents + (1 if c.defect == "segment_edge" else 0))
        a = c.seq_sum([c.rd(g, (b * Tt + P + p) * H + h) for p in range(p0, p1)], start=c.zeros(B, H))
        c.wr(out, (b * S + k) * H + h, a)


def k_embed_add(c, g, wpe, wte, type_ids, h, M, Tt, D, p, seed):
    m, d = _ar(M)[:, None], _ar(D)[None, :]
    t = (m // Tt) if c.defect == "pos_div" else (m % Tt)
    ty = c.ids(type_ids, m)
    v = c.rd(g, m * D + d) + c.rd(wpe, t * D + d) + c.rd(wte, ty * D + d)
    keep, ik = _keep(seed, (d + 0 * m) if c.defect == "drop_per_row" else (m * D + d), p)
    if hip.drop_thresh(p):
        v = fwhere(keep, v * c.const(float(np.float32(ik)), 0), c.zeros(M, D))      # (dropped elements are +0, whatever the sign of the sum)
    c.wr(h, m * D + d, v)


def k_embed_add_bwd(c, dh, type_ids, dwpe, dwte, M, Tt, D, ntypes, p, seed, atomic):
    m, d = _ar(M)[:, None], _ar(D)[None, :]
    x = c.rd(dh, m * D + d)
    if hip.drop_thresh(p):   # dh is masked in place first (mmtg_dropout_apply), the sums read the masked values as stored
        keep, ik = _keep(seed, m * D + d, p)
        x = fwhere(keep, x * c.const(float(np.float32(ik)), 0), 0.0 * x)
        c.wr(dh, m * D + d, x)
        if dh.dtype == BF:
            x = V(x.v.float().to(BF).double()) if c.ref else x.to(BF).float()   # (exact cases only: the reference rereads the store)
    Bn = M // Tt
    t = _ar(Tt)[:, None]
    c.wr(dwpe, t * D + d, c.rd(dwpe, t * D + d) + c.seq_sum([x[bb * Tt:(bb + 1) * Tt] for bb in range(Bn)]))
    ty = c.ids(type_ids, _ar(M))
    if c.defect == "type_fold":
        ty = torch.where((ty < 0) | (ty >= ntypes), torch.zeros_like(ty), ty)
    nblk = _cdiv(M, 128)
    if c.defect == "row_block" and nblk > 1:
        nblk = 1
    for k in range(ntypes):
        bins = []
        for blk in range(nblk):
            rows = [r for r in range(blk * 128, min(M, blk * 128 + 128)) if int(ty[r]) == k]
            bins.append(c.seq_sum([x[r] for r in rows], start=c.zeros(D)))
        # (atomics in any order, or mmtg_colsum over the row blocks' bins onto what dwte holds: the same bound covers both)
        c.wr(dwte, k * D + d[0], c.any_sum(c.rd(dwte, k * D + d[0]), _stack(bins)))


def _stack(xs):
    return V(torch.stack([x.v for x in xs], -1), torch.stack([x.e for x in xs], -1)) if isinstance(xs[0], V) else torch.stack(xs, -1)


def k_dropout_apply(c, x, y, n, p, seed):
    i = _ar(n)
    keep, ik = _keep(seed, i, p)
    v = c.rd(x, i)
    c.wr(y, i, fwhere(keep, v * c.const(float(np.float32(ik)), 0), 0.0 * v))


def embed_condition_case(bf, E, two_sents, S, L, P, B=2, Vn=9):
    T = _T(bf)
    tab = _randn(Vn, E, seed=E + Vn)
    g = _gen(E + L + P + S)
    tid = torch.randint(1, Vn - 1, (B, max(P, 1)), generator=g)
    tg = torch.randint(1, Vn - 1, (B, L), generator=g)
    tg[0, 0], tg[-1, -1] = -1, Vn + 3                       # clamped to rows 0 and Vn - 1
    if P:
        tid[0, -1], tid[-1, 0] = Vn + 3, -1
    used = set(tg.clamp(0, Vn - 1).reshape(-1).tolist()) | (set(tid.clamp(0, Vn - 1).reshape(-1).tolist()) if P else set())
    for r in range(Vn):
        if r not in used:
            tab[r] = NAN                                    # table rows that no id names
    table = _rows(Vn, E, T, tab)
    topic_ids = _rows(B, P, I64, tid) if P else None
    targets = _rows(B, L, I64, tg)
    cvec, x = _rows(B * S, E, T, _randn(B * S, E, seed=E + 3)), _rows(B * (P + L), E, T, None)
    bufs = dict(table=table, topic_ids=topic_ids, targets=targets, c=cvec, x=x)

    def launch(p):
        hip.embed_condition(p("table"), p("topic_ids"), p("targets"), p("c"), p("x"), B, P, L, S, E, two_sents, Vn)
    name = "embed_condition %s E=%d two_sents=%d S=%d L=%d P=%d" % (T, E, two_sents, S, L, P)
    return Case("embed_condition", name, bufs, lambda c: k_embed_condition(c, table, topic_ids, targets, cvec, x, B, P, L, S, E, two_sents, Vn), launch, exact=True)


def embed_condition_cases(bf):
    out = []
    for n, E in enumerate([8, 1016, 1024, 1032, 2040, 2048, 2056]):
        for two_sents, S in ((1, 1), (3, 2), (1, 2), (3, 1)):
            full = S * two_sents
            for L in sorted({max(1, two_sents - 1), full, full + 1}):       # inside one segment, an exact multiple, one past
                out.append(embed_condition_case(bf, E, two_sents, S, L, P=(0 if (n + L) % 2 else 2)))
    return out


def segment_sum_case(bf, H, P, L, S, two_sents, integer, B=2):
    T = _T(bf)
    gd = _ints(-8, 8, B * (P + L), H, seed=H + L) if integer else _randn(B * (P + L), H, seed=H + L)
    g, out = _rows(B * (P + L), H, T, gd), _rows(B * S, H, T, None)
    bufs = dict(g=g, out=out)

    def launch(p):
        hip.segment_sum(p("g"), p("out"), B, P, L, S, H, two_sents)

    def extra(after):        # an empty segment holds exact +0
        o = after["out"][PAD:PAD + out.n].view(B, S, H)
        for k in range(S):
            if k * two_sents >= L:
                assert bool((_bits(o[:, k]) == 0).all()), "empty segment %d" % k
    name = "segment_sum %s H=%d P=%d L=%d S=%d two_sents=%d %s" % (T, H, P, L, S, two_sents, "integer" if integer else "random")
    return Case("segment_sum", name, bufs, lambda c: k_segment_sum(c, g, out, B, P, L, S, H, two_sents), launch,
                exact="integer" if integer else False, extra=extra)


def segment_sum_cases(bf):
    out = []
    for H in (1, 255, 256, 257):
        for P in (0, 3):
            for integer in (True, False):
                out.append(segment_sum_case(bf, H, P, 7, 4, 3, integer))       # segments of 3, 3, 1 (ragged) and 0 (empty) rows
                out.append(segment_sum_case(bf, H, P, 11, 2, 4, integer))      # rows 8 .. 10 belong to no segment
    return out


def embed_add_case(bf, B, Tt, D, p, inplace=False, ntypes=5):
    T, M = _T(bf), B * Tt
    gd = _randn(M, D, seed=D + Tt)
    ty = torch.randint(0, ntypes, (M,), generator=_gen(D + M))
    ty[0], ty[-1] = ntypes - 1, ntypes - 1                  # the last wte row
    wpe, wte, type_ids = _rows(Tt, D, T, _randn(Tt, D, seed=D + 1)), _rows(ntypes, D, T, _randn(ntypes, D, seed=D + 2)), _rows(1, M, I64, ty)
    g = _rows(M, D, T, gd, operand=not inplace)
    h = g if inplace else _rows(M, D, T, None)
    bufs = dict(g=g, wpe=wpe, wte=wte, type_ids=type_ids)
    if not inplace:
        bufs["h"] = h

    def launch(pp):
        hip.embed_add(pp("g"), pp("wpe"), pp("wte"), pp("type_ids"), pp("g" if inplace else "h"), M, Tt, D, drop_p=p, drop_seed=SEED)

    def extra(after):        # dropped elements are +0
        keep, _ = _keep(SEED, _ar(M * D), p)
        o = after["g" if inplace else "h"][PAD:PAD + M * D]
        assert bool((_bits(o)[~keep] == 0).all())
    name = "embed_add %s B=%d T=%d D=%d p=%g%s" % (T, B, Tt, D, p, " in place" if inplace else "")
    return Case("embed_add", name, bufs, lambda c: k_embed_add(c, g, wpe, wte, type_ids, h, M, Tt, D, p, SEED), launch, exact=True, extra=extra)


def embed_add_cases(bf):
    out = []
    for n, D in enumerate((4, 768, 1020, 1024, 1028)):
        for p in (0.0, 0.1, 0.5):
            out.append(embed_add_case(bf, 3, 5, D, p, inplace=(n + int(p * 10)) % 2 == 1))
    return out


def embed_add_bwd_case(bf, B, Tt, D, ntypes, p, atomic, integer=True):
    T, M = _T(bf), B * Tt
    dd = _ints(-4, 4, M, D, seed=D + M + ntypes) if integer else _randn(M, D, seed=D + M + ntypes)
    ty = torch.randint(0, ntypes, (M,), generator=_gen(M + ntypes))
    ty[0], ty[M // 2], ty[-1] = -1, ntypes, ntypes - 1      # out of range: counted in dwpe, skipped in dwte
    if M > 128:
        ty[128] = ntypes - 1                                # the second row block holds a row of the last type
    dh = _rows(M, D, T, dd, operand=not hip.drop_thresh(p))
    type_ids = _rows(1, M, I64, ty)
    dwpe, dwte = _acc(_ints(-3, 3, Tt * D, seed=5)), _acc(_ints(-3, 3, ntypes * D, seed=6))
    bufs = dict(dh=dh, type_ids=type_ids, dwpe=dwpe, dwte=dwte)

    def launch(pp):
        if atomic:
            _rc(hip.lib().mmtg_embed_add_bwd(hip.dt(pp("dh")), _ptr(pp("dh")), _ptr(pp("type_ids")), _ptr(pp("dwpe")), _ptr(pp("dwte")), M, Tt, D, ntypes,
                                             hip.drop_thresh(p), SEED, 0, 0, _stream()), "embed_add_bwd (atomic form)")
        else:
            hip.embed_add_bwd(pp("dh"), pp("type_ids"), pp("dwpe"), pp("dwte"), M, Tt, D, ntypes, drop_p=p, drop_seed=SEED)

    def extra(after):        # an element of the masked dh is zero exactly where embed_add with the same seed drops it
        if hip.drop_thresh(p):
            keep, _ = _keep(SEED, _ar(M * D), p)
            o = after["dh"][PAD:PAD + M * D]
            src = dh.host[PAD:PAD + M * D]
            assert bool((o[~keep] == 0).all()) and bool(((o != 0) == (keep & (src != 0))).all())
            ik = torch.tensor(4294967296.0 / (4294967296.0 - float(hip.drop_thresh(p)))).float()
            _same_bits(name + " masked dh", o, torch.where(keep, src.float() * ik, src.float() * 0.0).to(T))
    name = "embed_add_bwd %s B=%d T=%d D=%d ntypes=%d p=%g %s %s" % (T, B, Tt, D, ntypes, p, "atomic" if atomic else "workspace", "integer" if integer else "random")
    # integer dh with p = 0.5 stays exact (the scale is 2); with p = 0.1 the masked dh is a single rounding and the sums are bounded
    exact = ("integer" if p in (0.0, 0.5) else False) if integer else False
    return Case("embed_add_bwd " + ("atomic" if atomic else "workspace"), name, bufs,
                lambda c: k_embed_add_bwd(c, dh, type_ids, dwpe, dwte, M, Tt, D, ntypes, p, SEED, atomic), launch, exact=exact, extra=extra)


EAB_BT = [(1, 128), (3, 43), (2, 128), (1, 257), (4, 96)]


def embed_add_bwd_cases(bf, atomic):
    out = []
    for n, (B, Tt) in enumerate(EAB_BT):
        for k, D in enumerate((4, 252, 256, 260) + ((6,) if atomic else ())):
            ntypes = (1, 11, 32)[(n + k) % 3]
            out.append(embed_add_bwd_case(bf, B, Tt, D, ntypes, (0.0, 0.5, 0.1)[(n + 2 * k) % 3], atomic, integer=True))
        out.append(embed_add_bwd_case(bf, B, Tt, 260, (32, 1, 11)[n % 3], 0.1, atomic, integer=False))
    return out


def dropout_apply_case(bf, n, p, inplace):
    T = _T(bf)
    x = _rows(1, n, T, _randn(1, n, seed=n), operand=not inplace)
    y = x if inplace else _rows(1, n, T, None)
    bufs = dict(x=x) if inplace else dict(x=x, y=y)

    def launch(pp):
        hip.dropout_apply(pp("x"), pp("x" if inplace else "y"), n, p, SEED)
    return Case("dropout_apply", "dropout_apply %s n=%d p=%g%s" % (T, n, p, " in place" if inplace else ""), bufs,
                lambda c: k_dropout_apply(c, x, y, n, p, SEED), launch, exact=True)


def dropout_apply_cases(bf):
    return [dropout_apply_case(bf, 4096 * 256 + 5, 0.1, True), dropout_apply_case(bf, 1, 0.5, False), dropout_apply_case(bf, 1, 0.5, True),
            dropout_apply_case(bf, 257, 0.5, False)]


EMBED_FAMILIES = dict(embed_condition=embed_condition_cases, segment_sum=segment_sum_cases, embed_add=embed_add_cases,
                      embed_add_bwd_ws=lambda bf: embed_add_bwd_cases(bf, False), embed_add_bwd_atomic=lambda bf: embed_add_bwd_cases(bf, True),
                      dropout_apply=dropout_apply_cases)


# =====================================================================================================================
# 6. the CPU half: the float32 models through the same checks, the planted defects
# =====================================================================================================================
BOTH = pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])


@BOTH
@pytest.mark.parametrize("entry", CELL_ENTRIES)
def test_cell_model_passes(entry, bf):
    _run_cases(cell_cases(entry, bf), model=True)


@BOTH
@pytest.mark.parametrize("shape", alpha_cases(), ids=lambda s: "B%d-S%d-H%d-h%d-%s" % s)
def test_alpha_model_passes(shape, bf):
    _alpha_pair(bf, shape, _model_run)


@BOTH
@pytest.mark.parametrize("shape", BETA_SHAPES, ids=lambda s: "B%d-S%d-H%d" % s)
def test_beta_model_passes(shape, bf):
    B, S, H = shape
    _run_cases([beta_fwd_case(bf, B, S, H), beta_bwd_case(bf, B, S, H, False), beta_bwd_case(bf, B, S, H, True),
                beta_bwd_case(bf, B, S, H, False, integer=True), beta_bwd_case(bf, B, S, H, True, integer=True)], model=True)
    if shape == BETA_SHAPES[0]:
        _run_cases([beta_bwd_case(bf, 2, 17, 100, True)], model=True)


@BOTH
@pytest.mark.parametrize("family", sorted(EMBED_FAMILIES))
def test_embed_model_passes(family, bf):
    cases = EMBED_FAMILIES[family](bf)
    if family == "dropout_apply":
        cases = cases[1:]    # (the million-element case is the kernel's grid-stride trip: nothing for a model to learn there)
    _run_cases(cases, model=True)


# defect -> the case that must reject it (bf16 where the storage type is given as True)
DEFECTS = {
    "natural_stride": lambda: gru_fwd_case(False, 3, 100, "step"),            # a natural stride used where a step stride was given
    "ld_gh": lambda: gru_fwd_case(True, 2, 129, "gh0"),                       # ld_gh = 0 ignored
    "rz_swap": lambda: gru_bwd_case(False, 1, 8, "nat", True),                # r / z swapped
    "dgh_r": lambda: gru_bwd_case(True, 1, 256, "step", True),                # da r missing in dgh
    "carry_twice": lambda: gru_bwd_case(False, 1, 8, "nat", True, (0, "alias")),
    "last_slab": lambda: gru_bwd_case(False, 2, 129, "step", True, (3, None)),
    "dc_in": lambda: rnn_bwd_case(False, 1, 1, 8, "nat", True, 1),            # dc_in ignored
    "tail": lambda: gru_fwd_case(False, 3, 100, "nat"),                       # the B H tail not computed
    "alpha_scale": lambda: alpha_fwd_case(False, 1, 3, 8, 1),
    "head_offset": lambda: alpha_fwd_case(True, 3, 2, 16, 2),
    "dk_transposed": lambda: alpha_bwd_case(False, 1, 3, 8, 1, "random", 0.0, _prior(3, 5).reshape(-1)),
    "lane_tail": lambda: alpha_fwd_case(False, 1, 5, 72, 1),                  # the lanes past the last multiple of 64 dropped
    "fuser_bias": lambda: beta_fwd_case(False, 2, 2, 64),
    "dtopic_overwritten": lambda: beta_bwd_case(False, 2, 2, 64, False, integer=True),
    "segment_edge": lambda: segment_sum_case(False, 255, 3, 7, 4, 3, True),   # segment boundary off by one
    "id_clamp": lambda: embed_condition_case(True, 8, 1, 1, 2, 2),            # id clamp missing
    "pos_div": lambda: embed_add_case(False, 3, 5, 4, 0.0),                   # m / T for the position
    "drop_per_row": lambda: embed_add_case(True, 3, 5, 768, 0.5),             # dropout indexed per row
    "row_block": lambda: embed_add_bwd_case(False, 1, 257, 4, 11, 0.0, False),  # second row block of dwte dropped
    "type_fold": lambda: embed_add_bwd_case(False, 3, 43, 4, 11, 0.0, True),  # out-of-range type id folded into type 0
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_is_rejected(defect):
    case = DEFECTS[defect]()
    _verify(case, _model_run(case))                         # the model itself passes the case ...
    with pytest.raises(AssertionError) as info:             # ... and is rejected with the defect planted
        _verify(case, _model_run(case, defect))
    print("%s: rejected by %s" % (defect, str(info.value)[:200]))


def test_segment_edge_defect_is_rejected_by_embed_condition_too():
    case = embed_condition_case(False, 8, 3, 2, 7, 0)
    with pytest.raises(AssertionError):
        _verify(case, _model_run(case, "segment_edge"))


def test_enc_transcendental_yardsticks():
    """the measured terms of this file, beside test_gemm_ops_gpu.test_transcendental_yardsticks: the float32 CPU forms against float64
    over the arguments the cases produce.  sigmoid as 1 / (1 + exp(-x)) at every multiple of 1 / 16 up to +-ARG_MAX and at +-100 (the
    saturated case); exp over [SOFTMAX_ARG_MIN, 0] (the softmax arguments: score minus the row's largest; the peaked case reaches
    about -45); log over [LOG_ARG_MIN, 1] (the KL term's priors and probabilities).  The figures printed are the source of SIG_YARD,
    EXP_YARD and LOG_YARD; the assertion is against the allowance the kernels get."""
    x = torch.cat([torch.arange(-int(ARG_MAX) * 16, int(ARG_MAX) * 16 + 1, dtype=F64) / 16.0, torch.tensor([-100.0, 100.0], dtype=F64)])
    sig = float((fsig(x.float()).double() - torch.sigmoid(x)).abs().max())
    t = (torch.arange(0, int(-SOFTMAX_ARG_MIN) * 64 + 1, dtype=F64) / -64.0).float()
    ex = float(((torch.exp(t).double() - torch.exp(t.double())).abs() / torch.exp(t.double())).max())
    y = torch.exp(torch.arange(1, 69 * 64 + 1, dtype=F64) / -64.0).float()
    assert float(y.min()) >= LOG_ARG_MIN
    lg = float(((torch.log(y).double() - torch.log(y.double())).abs() / torch.log(y.double()).abs()).max())
    for name, got, yard in (("sigmoid", sig, SIG_YARD), ("exp", ex, EXP_YARD), ("log", lg, LOG_YARD)):
        print("float32 %s against float64: largest error / scale %.3e (yardstick %.3e, allowed %.3e)" % (name, got, yard, LIBM_FACTOR * yard))
        assert got <= LIBM_FACTOR * yard, (name, got)


def test_model_worst_ratios():
    """the largest err / allowed of each float32 model over one pass of the bounded cases (printed for docs/experiments.md)"""
    WORST.clear()
    for bf in (False, True):
        for entry in CELL_ENTRIES:
            _run_cases([c for c in cell_cases(entry, bf) if "B=3 H=100" in c.name], model=True)
        _alpha_pair(bf, (3, 5, 512, 4, "random"), _model_run)
        _alpha_pair(bf, (2, 5, 144, 2, "peaked"), _model_run)
        _run_cases([beta_fwd_case(bf, 9, 5, 100), beta_bwd_case(bf, 9, 5, 100, False), beta_bwd_case(bf, 9, 5, 100, True)], model=True)
        _run_cases(segment_sum_cases(bf)[:8], model=True)
    for fam in sorted(WORST):
        print("model worst err / allowed: %-28s %.3f" % (fam, WORST[fam]))
        assert WORST[fam] <= 1.0


# =====================================================================================================================
# the GPU half
# =====================================================================================================================
@pytest.fixture(scope="module", autouse=True)
def _report():
    """after the file's last test: the worst err / allowed of every family this process ran (docs/experiments.md quotes them)"""
    yield
    for fam in sorted(WORST):
        print("worst err / allowed: %-40s %.3f" % (fam, WORST[fam]))


@gpu
@BOTH
@pytest.mark.parametrize("entry", CELL_ENTRIES)
def test_cell(entry, bf):
    _run_cases(cell_cases(entry, bf))


@gpu
@BOTH
@pytest.mark.parametrize("shape", alpha_cases(), ids=lambda s: "B%d-S%d-H%d-h%d-%s" % s)
def test_alpha(shape, bf):
    _alpha_pair(bf, shape, _gpu_run)


@gpu
@BOTH
@pytest.mark.parametrize("shape", BETA_SHAPES, ids=lambda s: "B%d-S%d-H%d" % s)
def test_beta(shape, bf):
    B, S, H = shape
    _run_cases([beta_fwd_case(bf, B, S, H), beta_bwd_case(bf, B, S, H, True), beta_bwd_case(bf, B, S, H, True, integer=True)])
    for integer in (False, True):                           # the workspace form: within the bound (exact on integers), the same bits twice
        case = beta_bwd_case(bf, B, S, H, False, integer=integer)
        first, second = _gpu_run(case), _gpu_run(case)
        _verify(case, first)
        for k in first:
            assert torch.equal(_bits(first[k]), _bits(second[k])), case.name + ": two calls differ in " + k
    if shape == BETA_SHAPES[0]:
        _run_cases([beta_bwd_case(bf, 2, 17, 100, True)])    # 17 steps: the atomic form alone accepts them


@gpu
@BOTH
@pytest.mark.parametrize("family", sorted(EMBED_FAMILIES))
def test_embed(family, bf):
    for case in EMBED_FAMILIES[family](bf):
        first = _gpu_run(case)
        _verify(case, first)
        if family == "embed_add_bwd_ws":
            second = _gpu_run(case)
            for k in first:
                assert torch.equal(_bits(first[k]), _bits(second[k])), case.name + ": two calls differ in " + k


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _refusal(what, bf):
    """-> (case, call(p) -> rc): an accepted case's buffers handed to the entry with one argument its MMTG_REQUIRE rejects"""
    L_, s, T = hip.lib(), _stream, hip.F32 if not bf else hip.BF16
    if what in ("alpha S=9", "alpha H % heads"):
        S, H, heads = (9, 64, 1) if what == "alpha S=9" else (3, 64, 3)
        case = alpha_fwd_case(bf, 2, 8, 128, 1)             # (buffers larger than either refused shape would touch)
        fw = lambda p: L_.mmtg_alpha_attn_fwd(T, _ptr(p("qkv")), _ptr(p("prior")), _ptr(p("ctx")), _ptr(p("probs")), _ptr(p("kl")), 1, S, H, heads, s())   # noqa: E731
        bw = lambda p: L_.mmtg_alpha_attn_bwd(T, _ptr(p("qkv")), _ptr(p("prior")), _ptr(p("probs")), _ptr(p("qkv")), 0.0, _ptr(p("ctx")), 1, S, H, heads, s())   # noqa: E731
        return case, [fw, bw]
    if what == "embed_condition E % 8":
        case = embed_condition_case(bf, 16, 1, 1, 2, 2)
        return case, [lambda p: L_.mmtg_embed_condition(T, _ptr(p("table")), _ptr(p("topic_ids")), _ptr(p("targets")), _ptr(p("c")), _ptr(p("x")), 2, 2, 2, 1, 12, 1, 9, s())]
    if what == "fuser H=1028":
        case = beta_bwd_case(bf, 1, 1, 8, False)
        ks = ("topic", "img", "txt", "att_w", "a", "d_o", "dtopic", "dimg", "dtxt", "datt_w", "datt_b")
        return case, [lambda p: L_.mmtg_beta_fuse_fwd(T, _ptr(p("topic")), _ptr(p("img")), _ptr(p("txt")), _ptr(p("att_w")), _ptr(p("datt_b")), _ptr(p("dimg")), _ptr(p("dtopic")), 1, 1, 1028, s()),
                      lambda p: L_.mmtg_beta_fuse_bwd(T, *[_ptr(p(k)) for k in ks], 1, 1, 1028, 0, 0, s())]
    if what in ("beta workspace short", "beta workspace S=17"):
        S = 17 if what.endswith("17") else 2
        case = beta_bwd_case(bf, 2, S, 8, False)
        ks = ("topic", "img", "txt", "att_w", "a", "d_o", "dtopic", "dimg", "dtxt", "datt_w", "datt_b")
        need = int(L_.mmtg_beta_fuse_bwd_ws(2, S, 8)) - (1 if S == 2 else 0)
        ws = torch.full((need + 8,), NAN, device=DEV)
        return case, [lambda p: (L_.mmtg_beta_fuse_bwd(T, *[_ptr(p(k)) for k in ks], 2, S, 8, ws.data_ptr(), need, s()), bool(torch.isnan(ws).all()))]
    if what in ("embed_add_bwd ntypes=33", "embed_add_bwd M % T", "embed_add_bwd workspace short"):
        case = embed_add_bwd_case(bf, 3, 43, 4, 32, 0.5, False)       # with dropout: a refused call must not have masked dh either
        M, Tt, nt = (129, 43, 33) if "ntypes" in what else (128, 43, 32) if "M % T" in what else (129, 43, 32)
        need = int(L_.mmtg_embed_add_bwd_ws(129, 4, 32)) - (1 if "short" in what else 0)
        ws = torch.full((need + 8,), NAN, device=DEV)
        return case, [lambda p: (L_.mmtg_embed_add_bwd(T, _ptr(p("dh")), _ptr(p("type_ids")), _ptr(p("dwpe")), _ptr(p("dwte")), M, Tt, 4, nt,
                                                       hip.drop_thresh(0.5), SEED, ws.data_ptr(), need, s()), bool(torch.isnan(ws).all()))]
    if what == "embed_add D % 4":
        case = embed_add_case(bf, 3, 5, 4, 0.0)
        return case, [lambda p: L_.mmtg_embed_add(T, _ptr(p("g")), _ptr(p("wpe")), _ptr(p("wte")), _ptr(p("type_ids")), _ptr(p("h")), 15, 5, 2, 0, 0, s())]
    if what == "rnn kind=2":
        case = rnn_fwd_case(bf, 1, 1, 8, "nat")
        return case, [lambda p: L_.mmtg_rnn_cell_fwd(T, 2, _ptr(p("gi")), 32, _ptr(p("gh")), 32, _ptr(p("cp")), _ptr(p("h")), 8, _ptr(p("c")), _ptr(p("save")), 1, 8, s()),
                      lambda p: L_.mmtg_rnn_cell_bwd(T, 2, _ptr(p("h")), 8, 0, _ptr(p("save")), _ptr(p("cp")), _ptr(p("h")), 8, _ptr(p("c")), 0, _ptr(p("gi")), 32, 1, 8, s())]
    if what == "0 < ld_gh < G H":
        case = rnn_fwd_case(bf, 1, 2, 8, "nat")
        g = gru_fwd_case(bf, 2, 8, "nat")
        case.bufs.update({"g_" + k: v for k, v in g.bufs.items()})
        return case, [lambda p: L_.mmtg_rnn_cell_fwd(T, 1, _ptr(p("gi")), 32, _ptr(p("gh")), 31, _ptr(p("cp")), _ptr(p("h")), 8, _ptr(p("c")), _ptr(p("save")), 2, 8, s()),
                      lambda p: L_.mmtg_rnn_cell_fwd(T, 0, _ptr(p("gi")), 32, _ptr(p("gh")), 7, 0, _ptr(p("h")), 8, 0, 0, 2, 8, s()),
                      lambda p: L_.mmtg_gru_cell_fwd(T, _ptr(p("g_gi")), 24, _ptr(p("g_gh")), 23, _ptr(p("g_hp")), 8, _ptr(p("g_h")), 8, _ptr(p("g_save")), 2, 8, s())]
    raise KeyError(what)


REFUSALS = ["alpha S=9", "alpha H % heads", "embed_condition E % 8", "fuser H=1028", "beta workspace short", "beta workspace S=17",
            "embed_add_bwd ntypes=33", "embed_add_bwd M % T", "embed_add_bwd workspace short", "embed_add D % 4", "rnn kind=2", "0 < ld_gh < G H"]


@gpu
@BOTH
@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(what, bf):
    case, calls = _refusal(what, bf)
    for call in calls:
        got = {}

        def launch(p):
            got["rc"] = call(p)
        after = _gpu_run(case, launch)
        rc = got["rc"]
        if isinstance(rc, tuple):
            rc, ws_untouched = rc
            assert ws_untouched, what + ": the refused call wrote its workspace"
        assert rc != 0 and hip.lib().mmtg_last_error(), what + ": accepted"
        for k, hb in case.bufs.items():
            if hb is not None:
                assert torch.equal(_bits(after[k]), _bits(hb.host)), "%s: the refused call changed %s" % (what, k)
