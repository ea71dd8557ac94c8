"""mmtg_cl_fwd / mmtg_cl_bwd alone against the float64 reference of tests/cl_ref.py, on planted clusters (cl_ref.planted): every
pair's rho - 1 + s_ij is far outside the deciding gap, so no pair and no row is left out.  Shapes, margins and what each covers:
cl_ref.SHAPES.  Row strides wider than the row on hf (NaN behind the row: never read), keep (nonzero behind the row) and dhf (a
sentinel behind the row), dhf pre-filled with a gradient of realistic size, one zero row from L = 17 up."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import cl_ref as R  # noqa: E402
from mmtg_amd import hip  # noqa: E402

DEV = "cuda"
FORMS = {"f32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "f32_bf16": (torch.float32, torch.bfloat16)}
COEF, SENTINEL, PADW = 0.5, 7.0, 8


@functools.lru_cache(maxsize=None)
def _reference(shape, in_dtype, margin):
    B, P, L, D = shape
    hf, keep, zero = R.planted(shape, in_dtype)
    fw = R.forward(hf, keep, P, L, margin, float(B))
    live = torch.isfinite(fw["margin_dist"])
    if bool(live.any()):
        dist, gap = float(fw["margin_dist"].min()), float(fw["gap"][live].max())
        assert dist > 10.0 * gap and dist > 0.086, (dist, gap)
    assert not bool(R.gap_rows(fw).any())
    inc, E, rows = R.backward(fw, COEF)
    return hf, keep, zero, fw, inc, E, rows


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _within(name, got, ref, allow):
    err = (got.double() - ref).abs()
    assert bool((err <= allow).all()), "%s: %d outside the bound, worst err/allowed %.3g" % (
        name, int((err > allow).sum()), float((err / allow.clamp(min=1e-300)).max()))


def _device_inputs(shape, hf, keep, out_dtype):
    B, P, L, D = shape
    M, Tt = B * (P + L), P + L
    hd = torch.full((M, D + PADW), float("nan"), dtype=hf.dtype)
    hd[:, :D] = hf.reshape(M, D)
    kd = torch.full((B, Tt + 3), 9, dtype=torch.int32)
    kd[:, :Tt] = keep
    gen = torch.Generator().manual_seed(11 + L)
    pre = torch.full((M, D + PADW), SENTINEL, dtype=out_dtype)
    pre[:, :D] = (1e-3 * torch.randn(M, D, generator=gen)).to(out_dtype)
    return hd.to(DEV), kd.to(DEV), pre


def _fwd(shape, hd, kd, margin):
    B, P, L, D = shape
    M = B * (P + L)
    nan = lambda n: torch.full((n,), float("nan"), device=DEV)
    rinv, row, smp, cl = nan(M), nan(M), nan(B), nan(1)
    hip.cl_fwd(hd, D + PADW, kd, P + L + 3, margin, B, P, L, D, float(B), rinv, row, smp, cl)
    return rinv, row, smp, cl


@pytest.mark.parametrize("margin", R.MARGINS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_kernels_follow_the_rule(shape, form, margin):
    B, P, L, D = shape
    in_dtype, out_dtype = FORMS[form]
    hf, keep, zero, fw, inc, E, rows = _reference(shape, in_dtype, margin)
    M, Tt = B * (P + L), P + L
    hd, kd, pre = _device_inputs(shape, hf, keep, out_dtype)

    # ---- forward
    rinv, row, smp, cl = _fwd(shape, hd, kd, margin)
    print(shape, form, margin, "cl %.7f ref %.7f allow %.2e" % (float(cl), float(fw["cl"]), float(fw["allow_cl"])))
    _within("rinv", rinv.cpu(), fw["rinv"], fw["allow_rinv"])
    _within("cl_row", row.cpu(), fw["cl_row"], fw["allow_row"])
    _within("cl_sample", smp.cpu(), fw["cl_sample"], fw["allow_sample"])
    _within("cl", cl.cpu(), fw["cl"].reshape(1), fw["allow_cl"].reshape(1))
    outside = torch.ones(B, Tt, dtype=torch.bool)
    outside[:, P:] = ~fw["valid"]
    assert bool((rinv.cpu().view(B, Tt)[outside] == 0).all()) and bool((row.cpu().view(B, Tt)[outside] == 0).all())
    if zero is not None:
        assert float(rinv.cpu().view(B, Tt)[zero[0], P + zero[1]]) == 0.0 and float(row.cpu().view(B, Tt)[zero[0], P + zero[1]]) == 0.0
    if L >= 2:
        assert float(cl) > 0 and float(smp[0]) > 0                # pairs were planted active
    else:
        assert float(cl) == 0.0 and float(smp[0]) == 0.0
    if shape == (2, 3, 2, 32):
        assert float(smp[1]) == 0.0                               # two centres: the pair is inactive
    if B == 4:
        assert float(smp[2]) == 0.0 and float(smp[3]) == 0.0      # n_b = 1, n_b = 0
    again = _fwd(shape, hd, kd, margin)
    for a, b in zip((rinv, row, smp, cl), again):
        assert torch.equal(_bits(a), _bits(b))

    # ---- backward
    def bwd(coef):
        d = pre.clone().to(DEV)
        hip.cl_bwd(hd, D + PADW, kd, Tt + 3, rinv, margin, coef, B, P, L, D, d, D + PADW)
        return d.cpu()

    got = bwd(COEF)
    assert torch.equal(_bits(got[:, D:]), _bits(pre[:, D:])), "sentinel columns"
    g3, p3 = got[:, :D].reshape(B, Tt, D), pre[:, :D].reshape(B, Tt, D)
    assert torch.equal(_bits(g3[:, :P]), _bits(p3[:, :P])), "topic rows"
    gl, pl = g3[:, P:], p3[:, P:]
    assert torch.equal(_bits(gl[~rows]), _bits(pl[~rows])), "PAD rows, zero rows, samples with n_b < 2"
    if zero is not None:
        assert not bool(rows[zero[0], zero[1]])
    if B == 4:
        assert not bool(rows[2].any()) and not bool(rows[3].any()) and int(rows[1].sum()) == int(keep[1, P:].sum())
    want = pl.double() + inc
    allow = R.out_allow(pl.double(), inc, E, "f32" if out_dtype == torch.float32 else "bf16")
    _within("dhf", gl[rows], want[rows], allow[rows])
    if L >= 2:
        moved = (gl.double() - pl.double())[rows]
        assert float(moved.abs().max()) > 0.5 * float(inc.abs().max()) > 0
    else:
        assert torch.equal(_bits(got), _bits(pre))
    assert torch.equal(_bits(bwd(COEF)), _bits(got)), "a second launch gives other bits"
    assert torch.equal(_bits(bwd(0.0)), _bits(pre)), "coef = 0 must leave dhf as it is"
