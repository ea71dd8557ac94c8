"""The three kernels of the token-level unlikelihood term (csrc/loss.hip: ul_row_kernel, ul_sample_kernel, loss_bwd_ul_kernel) against
the float64 reference of tests/ul_ref.py, B = 2 throughout.

Shapes (ul_ref.geometries): V / Vpad / ld in (333, 336, 336), (333, 384, 400), (16392, 16392, 16392) with L in {3, 66}; (333, 384, 384)
with L in {258, 1024} -- one id past a 256-thread trip, all four trips -- and P in {0, 3} everywhere; plus (333, 335, 335) with L = 3,
which takes the kernel's scalar dense pass.  ul_ref.case plants, in every shape that can hold them: an id three times in a context, the
label in its own context, every default exclude id, candidates at column 0 (without a list), V - 1 and (V - 1) & ~7, an id >= V and a
negative id, an empty candidate set, a clamped candidate (1 - p about V e^-25) and one with 1 - p near 1e-3; first occurrences at the
wave and trip edges of the long contexts.  Every case runs with the default exclude list and without one.

Bounds: derived in ul_ref's docstring by counting rounded fp32 operations, with the 1 / (1 - p) amplification of g explicit and per
element, so no element is left out of any comparison -- the clamped candidate included, at its defined value.
tests/test_ul_cpu.py's yardstick runs a float32 restatement of the kernels through the same bounds on the same cases.
"""
import pytest
import torch

import ul_ref as R
from mmtg_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
SENT = 1234.0                # columns a kernel must leave alone (exact in bf16)
FORMS = ["f32-f32", "f32-bf16", "bf16-bf16", "bf16-inplace", "x3"]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _within(name, got, ref, allow):
    err = (got.double() - ref).abs()
    ok = err <= allow
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d/%d outside the bound, first at %s: got %.9g, ref %.9g, allowed %.3g; worst err/allowed %.3g" % (
            name, len(bad), ok.numel(), i, float(got[i]), float(ref[i]), float(allow[i]),
            float((err / allow.clamp(min=1e-300)).nan_to_num(nan=float("inf")).max())))


def _params(forms):
    out = []
    for V, Vpad, ld, L in R.geometries():
        for form in forms:
            if Vpad % 8 and form in ("x3", "bf16-inplace"):
                continue
            for P in R.PS:
                out.append(pytest.param((V, Vpad, ld), L, P, form, id="V%d-Vpad%d-ld%d-L%d-P%d-%s" % (V, Vpad, ld, L, P, form)))
    return out


def _device_case(V, Vpad, ld, L, P, bf, sentinel_past_vpad=False):
    x, topic, tg, lse, coef, pl = R.case(V, P, L, bf)
    ldl = 336 if Vpad % 8 else ld
    lg = torch.full((x.shape[0], ldl), NAN, dtype=x.dtype)
    lg[:, :V] = x
    if sentinel_past_vpad:
        lg[:, Vpad:] = SENT
    return lg, ldl, (None if topic is None else topic.to(DEV)), tg.to(DEV), lse.to(DEV), coef.to(DEV), pl


def _exclude(with_list):
    return torch.tensor(R.DEFAULT_EXCLUDE, dtype=torch.long, device=DEV) if with_list else None


def _planted_are_there(fw, pl, V, L, with_list):
    mask, n = fw["mask"], fw["n"]
    assert int(n[pl["empty"]]) == 0
    nm, nc = pl["near"]
    cm, cc = pl["clamped"]
    assert bool(mask[nm, nc]) and 5e-4 < float(fw["q"][nm, nc]) < 2e-3
    assert bool(fw["clamped"][cm, cc]) and float(fw["g"][cm, cc]) == 0.0
    assert bool(mask[:, V - 1].any()) and bool(mask[:, (V - 1) & ~7].any())
    assert bool(mask[:, 0].any()) != with_list                                   # column 0 is a candidate exactly without the list
    if with_list:
        assert not bool(mask[:, list(R.DEFAULT_EXCLUDE)].any())
    if L >= 66:
        assert int(n[pl["dup"]]) <= 6                                             # 301 three times among eight ids
        assert int(n[pl["out_of_range"]]) == int(n[pl["out_of_range"] - 3])       # V, -3 and V + 70000 added nothing to the context


# ---- 1
@pytest.mark.parametrize("shape,L,P,form", _params(["f32", "bf16"]))
def test_ul_forward(shape, L, P, form):
    """ul_row, S, ul_sample and ul; rows outside [P, Tt - 2] exactly 0; a second launch writes the same bits"""
    V, Vpad, ld = shape
    bf = form == "bf16"
    lg, ldl, topic, tg, lse, coef, pl = _device_case(V, Vpad, ld, L, P, bf)
    M = lg.shape[0]
    lgd = lg.to(DEV)
    for with_list in (True, False):
        fw = R.reference(V, P, L, bf, with_list)
        _planted_are_there(fw, pl, V, L, with_list)
        outs = []
        for launch in range(2):
            row, S = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
            smp, ul = torch.full((R.B,), NAN, device=DEV), torch.full((1,), NAN, device=DEV)
            hip.loss_ul_fwd(lgd, ldl, V, tg, lse, _exclude(with_list), R.B, P, L, float(R.B), row, S, smp, ul)
            outs.append([t.cpu() for t in (row, S, smp, ul)])
        row, S, smp, ul = outs[0]
        name = "V=%d ld=%d L=%d P=%d %s list=%s" % (V, ld, L, P, form, with_list)
        print(name, "ul = %.6f (ref %.6f), max n = %d" % (float(ul), float(fw["ul"]), int(fw["n"].max())))
        _within(name + " ul_row", row, fw["ul_row"], fw["allow_row"])
        _within(name + " S", S, fw["S"], fw["allow_S"])
        _within(name + " ul_sample", smp, fw["ul_sample"], fw["allow_sample"])
        _within(name + " ul", ul, fw["ul"].reshape(1), fw["allow_ul"].reshape(1))
        off = ~R.loss_rows(R.B, P, L)
        assert bool((_bits(row[off]) == 0).all()) and bool((_bits(S[off]) == 0).all()), name + ": rows outside the loss rows must be +0"
        assert float(row[pl["empty"]]) == 0.0 and float(S[pl["empty"]]) == 0.0
        for a, b in zip(*outs):
            assert torch.equal(_bits(a), _bits(b)), name + ": two launches differ"


# ---- 2
def _sentinel_out(M, Vpad, ldd, dtype):
    o = torch.full((M, ldd), NAN, dtype=dtype)
    o[:, Vpad:] = SENT
    return o


def _launch(form, lg, ldl, V, topic, tg, lse, coef, gscale, lm_coef, S, u, ex, P, L, Vpad, ldd, plain=False):
    """one backward launch in `form` on fresh outputs; returns CPU tensors (out,) or (hi, lo).  plain=True: mmtg_loss_bwd / _x3"""
    M = lg.shape[0]
    lgd = lg.to(DEV)
    if form == "x3":
        planes = hip.Planes(torch.stack([_sentinel_out(M, Vpad, ldd, BF)] * 2).to(DEV), M, Vpad, ld=ldd)
        if plain:
            hip.loss_bwd_x3(lgd, ldl, V, topic, tg, lse, coef, gscale, R.B, P, L, planes, Vpad, lm_coef=lm_coef)
        else:
            hip.loss_bwd_ul_x3(lgd, ldl, V, topic, tg, lse, coef, gscale, S, u, ex, R.B, P, L, planes, Vpad, lm_coef=lm_coef)
        return planes.t[0].cpu(), planes.t[1].cpu()
    out = lgd if form == "bf16-inplace" else _sentinel_out(M, Vpad, ldd, F32 if form == "f32-f32" else BF).to(DEV)
    if plain:
        hip.loss_bwd(lgd, ldl, V, topic, tg, lse, coef, gscale, R.B, P, L, out, ldd, Vpad, lm_coef=lm_coef)
    else:
        hip.loss_bwd_ul(lgd, ldl, V, topic, tg, lse, coef, gscale, S, u, ex, R.B, P, L, out, ldd, Vpad, lm_coef=lm_coef)
    return (out.cpu(),)


def _check_layout(name, got, V, Vpad, lm_coef, P, Tt):
    """exact zeros of pad columns and inactive rows, untouched columns past Vpad"""
    assert bool((_bits(got[:, V:Vpad]) == 0).all()), name + ": columns [V, Vpad) must be exactly +0"
    assert bool((_bits(got[:, Vpad:]) == _bits(torch.full((1,), SENT, dtype=got.dtype))).all()), name + ": columns past Vpad were written"
    t = torch.arange(got.shape[0]) % Tt
    inactive = (t == Tt - 1) | ((t < P) & (lm_coef == 0.0))
    assert bool((_bits(got[inactive][:, :Vpad]) == 0).all()), name + ": an inactive row is not all +0"
    assert bool((got[~inactive][:, :V] != 0).any(1).all()), name + ": an active row is all zero"


@pytest.mark.parametrize("shape,L,P,form", _params(FORMS))
def test_loss_bwd_ul(shape, L, P, form):
    """d(logits) in one storage form: every element against float64, zeros and untouched columns, the row with an empty candidate set
    and the whole tensor at u = 0 bit-equal to mmtg_loss_bwd's, two launches bit-equal"""
    V, Vpad, ldd = shape
    bf = form.startswith("bf16")
    lg, ldl, topic, tg, lse, coef, pl = _device_case(V, Vpad, ldd, L, P, bf, sentinel_past_vpad=form == "bf16-inplace")
    Tt = P + L
    out_form = "f32" if form == "f32-f32" else "bf16"
    for with_list in (True, False):
        fw = R.reference(V, P, L, bf, with_list)
        ex = _exclude(with_list)
        S32 = fw["S"].float()
        Sd = S32.to(DEV)
        for lm_coef, gscale in R.COMBOS:
            name = "%s V=%d Vpad=%d ldd=%d L=%d P=%d list=%s lm_coef=%g gscale=%g" % (form, V, Vpad, ldd, L, P, with_list, lm_coef, gscale)
            args = (lg, ldl, V, topic, tg, lse, coef, gscale, lm_coef, Sd)
            tail = (ex, P, L, Vpad, ldd)
            plain = _launch(form, *args, 0.0, *tail, plain=True)
            zero = _launch(form, *args, 0.0, *tail)
            for a, b in zip(plain, zero):
                assert torch.equal(_bits(a), _bits(b)), name + ": u = 0 differs from mmtg_loss_bwd, %d elements" % int((_bits(a) != _bits(b)).sum())
            got = _launch(form, *args, R.U, *tail)
            again = _launch(form, *args, R.U, *tail)
            for a, b in zip(got, again):
                assert torch.equal(_bits(a), _bits(b)), name + ": two launches differ"
            d, allow, rc = R.backward(fw, S32, None if topic is None else topic.cpu(), tg.cpu(), coef.cpu(), gscale, lm_coef, R.U, P, V)
            _within(name, got[0][:, :V], d, R.out_allow(d, allow, out_form))
            _check_layout(name, got[0], V, Vpad, lm_coef, P, Tt)
            if form == "x3":
                hi, lo = got
                _within(name + " hi + lo", (hi.double() + lo.double())[:, :V], d, R.out_allow(d, allow, "x3"))
                assert bool((_bits(lo[:, V:Vpad]) == 0).all()) and bool((_bits(lo[:, Vpad:]) == _bits(torch.full((1,), SENT, dtype=BF))).all())
                t = torch.arange(hi.shape[0]) % Tt
                assert bool((lo[(t == Tt - 1) | ((t < P) & (lm_coef == 0.0))][:, :Vpad] == 0).all()), name + ": lo plane of an inactive row"
            assert not torch.equal(_bits(got[0][pl["near"][0]]), _bits(plain[0][pl["near"][0]])), name + ": the term changed nothing"
            # a row without candidates: S = 0, nothing to fix up -- mmtg_loss_bwd's bits
            e = pl["empty"]
            for a, b in zip(got, plain):
                assert torch.equal(_bits(a[e]), _bits(b[e])), name + ": the row with an empty candidate set"


# ---- 3
def test_the_entries_refuse_on_the_device_path_too():
    """a context longer than the kernels stage, and a negative coefficient, raise before anything is launched"""
    V, L = 333, R.LONG_L[-1] + 1
    M = R.B * L
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=DEV)
    tg = torch.zeros(R.B, L, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match="at most 1024"):
        hip.loss_ul_fwd(z(M, 336), 336, V, tg, z(M), None, R.B, 0, L, 2.0, z(M), z(M), z(R.B), z(1))
    out = torch.full((M, 336), SENT, device=DEV)
    with pytest.raises(RuntimeError, match="at most 1024"):
        hip.loss_bwd_ul(z(M, 336), 336, V, None, tg, z(M), z(R.B), 1.0, z(M), 0.3, None, R.B, 0, L, out, 336, 336)
    with pytest.raises(RuntimeError, match="ul_coef"):
        hip.loss_bwd_ul(z(M, 336), 336, V, None, tg[:, :66].contiguous(), z(M), z(R.B), 1.0, z(M), -0.3, None, R.B, 0, 66, out, 336, 336)
    assert bool((out == SENT).all())
