"""Contrastive token loss on the last-layer states, the host side: the two entries' declarations and argument checks, the float64
reference of tests/cl_ref.py against a restatement of SimCTG's published loss under autograd, a float32 evaluation of the kernels'
expressions inside the reference's bounds on every case of tests/test_cl_ops_gpu.py, and the trainer's arguments.  No GPU."""
import ctypes
import fnmatch
import os
import re

import pytest
import torch

import cl_ref as R
from mmtg_amd import hip
from mmtg_amd.trainer import MMTGTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmtg_cl_fwd", "mmtg_cl_bwd")


# ---- 1
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    exports = open(os.path.join(ROOT, "mmtg_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    lib = ctypes.CDLL(hip.lib_path())
    for name in ENTRIES:
        assert name + "(" in header and name in hip.exported_symbols() and name in hip._SIGS and hasattr(lib, name)
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), (name, patterns)
    assert [len(hip._SIGS[n][0]) for n in ENTRIES] == [16, 16]
    assert hip.lib().mmtg_abi_version() == hip.ABI_VERSION == 12
    assert "#define MMTG_ABI_VERSION 12" in header and "MMTG_CL_MAX_L 1024" in header and "MMTG_CL_MAX_D 1024" in header
    assert callable(hip.cl_fwd) and callable(hip.cl_bwd) and (hip.CL_MAX_L, hip.CL_MAX_D) == (1024, 1024)


# ---- 2: fake device addresses: every case is refused on the host, before any device call, so no GPU is touched
A = [0x7000000000 + 0x100000000 * i for i in range(8)]
NAN, INF = float("nan"), float("inf")


def _refused(fn, prefix, args, what, match):
    assert fn(*args) != 0, what
    err = hip.lib().mmtg_last_error().decode()
    assert err.startswith(prefix + ": "), (what, err)
    assert match in err, (what, err)


def _each(fn, prefix, good, bad):
    for what, (i, v, match) in bad.items():
        args = list(good)
        for k, val in zip(i if isinstance(i, tuple) else (i,), v if isinstance(i, tuple) else (v,)):
            args[k] = val
        _refused(fn, prefix, args, what, match)


def test_cl_fwd_checks_its_arguments():
    #       dtype hf  ldh  keep  ldkeep margin B  P  L   D   den  rinv  row   sample cl   stream
    good = [1, A[0], 72, A[1], 40, 0.5, 2, 3, 33, 64, 2.0, A[2], A[3], A[4], A[5], None]
    bad = {"dtype": (0, 7, "dtype"), "null hf": (1, None, "hf"), "ldh < D": (2, 56, "ldh"), "ldh % 8 (bf16 rows)": (2, 68, "hf rows"),
           "ldh % 4 (f32 rows)": ((0, 2), (0, 66), "hf rows"), "misaligned hf": (1, A[0] + 8, "hf rows"), "null keep": (3, None, "keep"),
           "misaligned keep": (3, A[1] + 2, "keep"), "ldkeep < P + L": (4, 35, "ldkeep"), "margin 0": (5, 0.0, "margin"),
           "margin > 1": (5, 1.5, "margin"), "margin < 0": (5, -0.5, "margin"), "margin nan": (5, NAN, "margin"), "B = 0": (6, 0, "B="),
           "P < 0": (7, -1, "P="), "L = 0": (8, 0, "L ="), "L = 1025": ((8, 4), (1025, 2000), "L ="), "D = 48": (9, 48, "D ="),
           "D = 0": (9, 0, "D ="), "D = 1056": ((9, 2), (1056, 1056), "D ="), "batch_den 0": (10, 0.0, "batch_den"),
           "batch_den nan": (10, NAN, "batch_den"), "batch_den inf": (10, INF, "batch_den"), "null rinv": (11, None, "rinv"),
           "null cl_row": (12, None, "cl_row"), "null cl_sample": (13, None, "cl_sample"), "null cl": (14, None, "cl")}
    _each(hip.lib().mmtg_cl_fwd, "cl_fwd", good, bad)


def test_cl_bwd_checks_its_arguments():
    #       dtype out hf   ldh  keep  ldkeep rinv margin coef B  P  L   D   dhf   ldd stream
    good = [0, 1, A[0], 68, A[1], 40, A[2], 0.5, 0.5, 2, 3, 33, 64, A[3], 72, None]
    bad = {"dtype": (0, 7, "dtype"), "out_dtype": (1, 5, "out_dtype"), "bf16 hf into f32 dhf": ((0, 1, 3), (1, 0, 72), "out_dtype"),
           "null hf": (2, None, "hf"), "ldh < D": (3, 60, "ldh"), "ldh % 4": (3, 66, "hf rows"), "misaligned hf": (2, A[0] + 4, "hf rows"),
           "null keep": (4, None, "keep"), "ldkeep < P + L": (5, 35, "ldkeep"), "null rinv": (6, None, "rinv"), "margin 0": (7, 0.0, "margin"),
           "margin 1.01": (7, 1.01, "margin"), "margin nan": (7, NAN, "margin"), "coef < 0": (8, -0.1, "coef"), "coef nan": (8, NAN, "coef"),
           "coef inf": (8, INF, "coef"), "B = 0": (9, 0, "B="), "P < 0": (10, -2, "P="), "L = 0": (11, 0, "L ="),
           "L = 1025": ((11, 5), (1025, 2000), "L ="), "D = 80": (12, 80, "D ="), "D = 2048": ((12, 3, 14), (2048, 2048, 2048), "D ="),
           "null dhf": (13, None, "dhf"), "ldd < D": (14, 56, "ldd"), "ldd % 8 (bf16 rows)": (14, 68, "dhf rows"),
           "ldd % 4 (f32 rows)": ((1, 14), (0, 66), "dhf rows"), "misaligned dhf": (13, A[3] + 2, "dhf rows")}
    _each(hip.lib().mmtg_cl_bwd, "cl_bwd", good, bad)


# ---- 3: SimCTG's contrastive_loss (Su et al., 2022: a cosine score matrix, gold score 1 on the diagonal, relu(margin - (gold - score)),
# the PAD mask), restated in float64 with per-sample normalisation, under autograd
def _simctg(hf, keep, P, margin, batch_den):
    h = hf[:, P:]
    valid = (keep[:, P:] != 0).double()
    norm = h.norm(dim=-1, keepdim=True)
    rep = torch.where(norm > 0, h / norm.clamp(min=1e-300), torch.zeros_like(h))
    score = rep @ rep.transpose(1, 2)
    gold = torch.ones_like(score[:, :, :1])
    loss = torch.relu(margin - (gold - score))
    L = h.shape[1]
    mask = valid[:, :, None] * valid[:, None, :] * (1.0 - torch.eye(L, dtype=torch.float64))[None]
    n = valid.sum(-1)
    per = (loss * mask).sum((1, 2)) / (n * (n - 1)).clamp(min=1.0)
    per = torch.where(n >= 2, per, torch.zeros_like(per))
    return per, per.sum() / batch_den


@pytest.mark.parametrize("shape", R.SHAPES[:5])
@pytest.mark.parametrize("margin", R.MARGINS)
def test_the_reference_is_simctg_s_loss(shape, margin):
    B, P, L, D = shape
    hf, keep, _ = R.planted(shape, torch.float32, seed=3)
    fw = R.forward(hf, keep, P, L, margin, float(B))
    inc, _, rows = R.backward(fw, 0.75)
    x = hf.double().requires_grad_(True)
    per, cl = _simctg(x, keep, P, float(torch.tensor(margin, dtype=torch.float32)), float(B))
    (0.75 * per.sum()).backward()
    assert float((fw["cl_sample"] - per.detach()).abs().max()) <= 1e-12 and abs(float(fw["cl"] - cl.detach())) <= 1e-12
    g = x.grad
    assert float((g[:, P:] - inc).abs().max()) <= 1e-12 and float(g[:, :P].abs().sum()) == 0.0
    assert bool((g[:, P:][~rows] == 0).all())
    if L >= 2:
        assert float(fw["cl"]) > 0 and float(inc.abs().max()) > 0


# ---- 4: the kernels' expressions evaluated in float32 on the host stay inside the bounds, on every case of the GPU file
def _f32_eval(hf, keep, P, margin, batch_den, coef):
    f = torch.float32
    h = hf.to(f)[:, P:]
    valid = keep[:, P:] != 0
    q = (h * h).sum(-1)
    rinv = torch.where(valid & (q > 0), 1.0 / q.sqrt(), torch.zeros_like(q))
    s = (h @ h.transpose(1, 2)) * (rinv[:, :, None] * rinv[:, None, :])
    x = torch.tensor(margin, dtype=f) - 1.0 + s
    L = h.shape[1]
    on = (rinv[:, :, None] > 0) & (rinv[:, None, :] > 0) & ~torch.eye(L, dtype=torch.bool)[None] & (x > 0)
    row = torch.where(on, x, torch.zeros_like(x)).sum(-1)
    n = valid.sum(-1).to(f)
    smp = torch.where(n >= 2, row.sum(-1) / (n * (n - 1)).clamp(min=1.0), torch.zeros_like(n))
    cl = smp.sum() / torch.tensor(batch_den, dtype=f)
    u = h * rinv[..., None]
    scale = torch.where(n >= 2, 2.0 / (n * (n - 1)).clamp(min=1.0), torch.zeros_like(n))[:, None, None]
    g = (on.to(f) @ u) * scale
    p = (g * u).sum(-1, keepdim=True)
    inc = (torch.tensor(coef, dtype=f) * rinv[..., None]) * (g - p * u)
    return rinv, row, smp, cl, inc


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_float32_evaluation_is_inside_the_bounds(shape, dtype):
    B, P, L, D = shape
    for margin in R.MARGINS:
        hf, keep, _ = R.planted(shape, dtype)
        fw = R.forward(hf, keep, P, L, margin, float(B))
        inc, E, rows = R.backward(fw, 0.5)
        assert not bool(R.gap_rows(fw).any())
        rinv, row, smp, cl, i32 = _f32_eval(hf, keep, P, margin, float(B), 0.5)
        lyr = lambda v: v.reshape(B, P + L)[:, P:]
        assert bool(((rinv.double() - lyr(fw["rinv"])).abs() <= lyr(fw["allow_rinv"])).all())
        assert bool(((row.double() - lyr(fw["cl_row"])).abs() <= lyr(fw["allow_row"])).all())
        assert bool(((smp.double() - fw["cl_sample"]).abs() <= fw["allow_sample"]).all())
        assert abs(float(cl) - float(fw["cl"])) <= float(fw["allow_cl"])
        assert bool(((i32.double() - inc).abs() <= E).all()), float(((i32.double() - inc).abs() / E.clamp(min=1e-300)).max())
        # ... and the bound is a bound on fp32 work, not room for a bf16 rounding of u_j: that is up to 2^-8 per term before the projection
        if L >= 17:
            u16 = fw["u"].to(torch.bfloat16).double()
            g = (fw["act"].double() @ u16) * (2.0 / (fw["n"].double() * (fw["n"].double() - 1)).clamp(min=1.0))[:, None, None]
            t = (g - (g * fw["u"]).sum(-1, keepdim=True) * fw["u"]) * 0.5 * fw["rinv_l"][..., None]
            bad = ((t - inc).abs() > E) & rows[..., None]
            assert float(bad.double().mean()) > 0.2, float(bad.double().mean())


# ---- 5: the trainer's arguments (refused before the model is touched)
@pytest.mark.parametrize("kw,name", [({"cl_weight": -0.1}, "cl_weight"), ({"cl_weight": NAN}, "cl_weight"), ({"cl_weight": INF}, "cl_weight"),
                                     ({"cl_weight": "0.5"}, "cl_weight"), ({"cl_weight": True}, "cl_weight"), ({"cl_margin": 0.0}, "cl_margin"),
                                     ({"cl_margin": 1.5}, "cl_margin"), ({"cl_margin": NAN}, "cl_margin"), ({"cl_margin": None}, "cl_margin"),
                                     ({"cl_margin": "0.5"}, "cl_margin"), ({"cl_margin": -0.5}, "cl_margin")])
def test_the_trainer_validates_its_arguments(kw, name):
    with pytest.raises(ValueError, match=name):
        MMTGTrainer(None, **kw)
