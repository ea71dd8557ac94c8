"""The per-modality guided validation loss, the host side: mmtg_guided_loss_multi's declaration and argument checks, the trainer's
arguments and best_scale, and a float32 evaluation of the kernel's expressions inside the bounds of tests/mgl_ref.py on every case of
tests/test_mgloss_ops_gpu.py.  No GPU."""
import ctypes
import fnmatch
import inspect
import os
import re

import pytest
import torch

import cfg_ref
import mgl_ref as R
from mmtg_amd import hip
from mmtg_amd.engine import Engine
from mmtg_amd.trainer import MMTGTrainer, best_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mmtg_guided_loss_multi"
NAN, INF = float("nan"), float("inf")


# ---- 1
def test_the_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    exports = open(os.path.join(ROOT, "mmtg_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    lib = ctypes.CDLL(hip.lib_path())
    assert NAME + "(" in header and NAME in hip.exported_symbols() and NAME in hip._SIGS and hasattr(lib, NAME)
    assert any(fnmatch.fnmatchcase(NAME, p.strip()) for p in patterns), patterns
    assert len(hip._SIGS[NAME][0]) == 17
    assert hip.lib().mmtg_abi_version() == hip.ABI_VERSION == 12 and "#define MMTG_ABI_VERSION 12" in header
    assert "#define MMTG_GUIDED_MAX_SCALES 8" in header and "#define MMTG_GUIDED_MAX_BRANCHES 4" in header
    assert hip.GUIDED_MAX_SCALES == R.MAX_TUPLES == 8 and hip.GUIDED_MAX_BRANCHES == R.MAX_BRANCHES == 4
    assert callable(hip.guided_loss_multi) and callable(Engine.guided_loss_multi)
    assert list(inspect.signature(hip.guided_loss_multi).parameters) == [
        "mats", "lses", "ldl", "V", "targets", "scale_tuples", "B", "P", "L", "batch_den", "nll", "sample_ce", "ce"]
    assert list(inspect.signature(Engine.guided_loss_multi).parameters) == ["self", "scale_tuples", "neg_logits", "neg_lses", "batch_den"]


# ---- 2: fake device addresses: every case is refused on the host, before any device call, so no GPU is touched
A = [0x7000000000 + 0x100000000 * i for i in range(14)]
_keep = []


def _ptrs(*addrs):
    arr = (ctypes.c_void_p * 4)(*addrs)
    _keep.append(arr)
    return ctypes.addressof(arr)


def _floats(*v):
    arr = (ctypes.c_float * 24)(*(v + (1.0,) * (24 - len(v))))
    _keep.append(arr)
    return ctypes.addressof(arr)


def _refused(args, what, match):
    assert hip.lib().mmtg_guided_loss_multi(*args) != 0, what
    err = hip.lib().mmtg_last_error().decode()
    assert err.startswith("guided_loss_multi: "), (what, err)
    assert match in err, (what, err)


def test_guided_loss_multi_checks_its_arguments():
    X, Ls, S = _ptrs(A[0], A[1], A[2], A[3]), _ptrs(A[4], A[5], A[6], A[7]), _floats(0.0, 1.0, 1.5, 2.0, 3.0, 7.5)
    # M = 2 * 8 = 16 rows, nll [8, 16]
    #       ldt logits lse K ldl  V    targets scales G B P L  den  nll   smp    ce     stream
    good = [1, X, Ls, 4, 168, 160, A[8], S, 8, 2, 3, 5, 2.0, A[9], A[10], A[11], None]
    with_ = lambda k, p, base=(A[0], A[1], A[2], A[3]): _ptrs(*[p if i == k else a for i, a in enumerate(base)])
    lse_with = lambda k, p: with_(k, p, (A[4], A[5], A[6], A[7]))
    mat_bytes = (15 * 168 + 160) * 2
    bad = {"dtype": (0, 5, "dtype"), "null logits": (1, None, "logits"), "null lse": (2, None, "lse"), "null targets": (6, None, "targets"),
           "null scales": (7, None, "scales"), "null nll": (13, None, "nll"), "null sample_ce": (14, None, "sample_ce"), "null ce": (15, None, "ce"),
           "K = 1": (3, 1, "K ="), "K = 5": (3, 5, "K ="), "K = 0": (3, 0, "K ="), "K < 0": (3, -2, "K ="),
           "G = 0": (8, 0, "G ="), "G = 9": (8, 9, "G ="), "G < 0": (8, -1, "G ="),
           "scale nan": (7, _floats(1.0, NAN), "scale 1 of tuple 0"), "scale inf": (7, _floats(1.0, 1.0, 1.0, INF), "scale 0 of tuple 1"),
           "scale < 0": (7, _floats(*([1.0] * 23 + [-0.5])), "scale 2 of tuple 7"),
           "V = 0": (5, 0, "V ="), "V < 0": (5, -4, "V ="), "ldl < V": (4, 152, "ldl"), "bf16 ldl % 8": (4, 164, "bf16 rows"),
           "B = 0": (9, 0, "B ="), "P < 0": (10, -1, "P ="), "L = 1": (11, 1, "L ="), "L = 0": (11, 0, "L ="),
           "batch_den 0": (12, 0.0, "batch_den"), "batch_den < 0": (12, -2.0, "batch_den"), "batch_den nan": (12, NAN, "batch_den"),
           "batch_den inf": (12, INF, "batch_den")}
    for k in range(4):
        bad["null logits[%d]" % k] = (1, with_(k, None), "logits[%d]" % k)
        bad["null lse[%d]" % k] = (2, lse_with(k, None), "lse[%d]" % k)
        bad["misaligned bf16 matrix %d" % k] = (1, with_(k, A[k] + 8), "bf16 rows")
        bad["misaligned f32 matrix %d" % k] = ((0, 1), (0, with_(k, A[k] + 2)), "fp32 rows")
        bad["nll is matrix %d" % k] = (13, A[k], "nll overlaps logits matrix %d" % k)
        bad["nll starts in the last row of matrix %d" % k] = (13, A[k] + mat_bytes - 2, "nll overlaps logits matrix %d" % k)
        bad["nll ends in matrix %d" % k] = (13, A[k] - 8 * 16 * 4 + 4, "nll overlaps logits matrix %d" % k)
    for what, (i, v, match) in bad.items():
        args = list(good)
        for j, val in zip(i if isinstance(i, tuple) else (i,), v if isinstance(i, tuple) else (v,)):
            args[j] = val
        _refused(args, what, match)
    # what lies behind the K and G that are read is not looked at: a null in slot 3 at K = 3, a NaN behind the G (K - 1) scales
    ok = list(good)
    ok[1], ok[2], ok[3], ok[7], ok[8], ok[11] = with_(3, None), lse_with(3, None), 3, _floats(1.0, 2.0, 3.0, 4.0, NAN), 2, 1
    _refused(ok, "K = 3, G = 2 beside a null and a NaN behind them: L is what is refused", "L =")
    # nll directly behind a matrix's last read logit, and directly in front of a matrix, overlaps nothing
    for addr in (A[3] + mat_bytes, A[0] - 8 * 16 * 4):
        edge = list(good)
        edge[13], edge[11] = addr, 1
        _refused(edge, "nll beside a matrix is not what is refused", "L =")


# ---- 3: the trainer's arguments (refused before anything of the trainer is touched) and best_scale
def test_scale_triples_are_refused_as_check_modality_guidance_refuses_them():
    tr = MMTGTrainer.__new__(MMTGTrainer)
    for fn in (lambda s: tr.evaluate_modality_guided_batch({}, s), lambda s: tr.evaluate_modality_guided([], s)):
        for bad in ([], [(1, 1, 1)] * 9, "12", b"12", 3.0, None, [1.0, 2.0, 3.0], [(1, 1)], [(1, 1, 1, 1)], ["abc"], [None], [3.0],
                    [(1, 1, 1), (1, 2)]):
            with pytest.raises(ValueError, match="scales"):
                fn(bad)
        for bad, arg in (((NAN, 1, 1), "guidance_scale"), ((1, -0.5, 1), "image_guidance_scale"), ((1, 1, INF), "text_guidance_scale"),
                         ((1, "2", 1), "image_guidance_scale"), ((1, 1, True), "text_guidance_scale"), ((None, 1, 1), "guidance_scale")):
            with pytest.raises(ValueError, match=r"^" + arg + " must be"):
                fn([(1, 1, 1), bad])
    from mmtg_amd.trainer import _check_scale_triples
    got = _check_scale_triples([(1, 2, 0.5), [0, 1, 1]])
    assert got == [(1.0, 2.0, 0.5), (0.0, 1.0, 1.0)] and all(type(v) is float for t in got for v in t)
    for name in ("evaluate_modality_guided_batch", "evaluate_modality_guided"):
        p = inspect.signature(getattr(MMTGTrainer, name)).parameters
        assert list(p)[:3] == ["self", "batch" if name.endswith("batch") else "valid_batches", "scales"] and p["stage"].default == 3
    assert inspect.signature(MMTGTrainer.evaluate_modality_guided).parameters["averaged"].default is False
    assert inspect.signature(MMTGTrainer.evaluate_modality_guided_batch).parameters["filter_rows"].default is True


def test_best_scale():
    single = {"scales": [0.0, 1.0, 2.0], "ce": [3.0, 2.5, 2.75], "ce_cond": 2.5, "ce_uncond": 3.0, "rows": 5}
    assert best_scale(single) == 1.0 and type(best_scale(single)) is float
    triples = {"scales": [(1.0, 1.0, 1.0), (1.0, 2.0, 1.5), (1.0, 3.0, 1.0)], "ce": [2.5, 2.25, 2.4], "ce_cond": 2.5, "ce_negatives": {}, "rows": 7}
    assert best_scale(triples) == (1.0, 2.0, 1.5) and best_scale(triples)[1:] == (2.0, 1.5)
    assert best_scale(dict(single, ce=[2.5, 2.5, 2.75])) == 0.0                   # the first of equal minima
    assert best_scale(dict(triples, ce=[2.5, 2.25, 2.25])) == (1.0, 2.0, 1.5)
    assert best_scale(dict(single, ce=[2.75, 2.5, 2.5])) == 1.0
    for bad in (dict(single, rows=0, ce=[0.0] * 3), dict(triples, rows=0, ce=[0.0] * 3), dict(single, ce=[3.0, NAN, 2.0]),
                dict(single, ce=[3.0, 2.0, INF]), dict(triples, ce=[-INF, 2.0, 2.0])):
        with pytest.raises(ValueError, match="best_scale"):
            best_scale(bad)


# ---- 4: the kernel's expressions in float32 stay inside the bounds, on every case of the GPU file
@pytest.mark.parametrize("geo", R.geometries(), ids=R.geo_id)
def test_a_float32_evaluation_is_inside_the_bounds(geo):
    V, ldl, P, L, bf, off = geo
    rows = cfg_ref.loss_rows(R.B, P, L)
    for K in R.KS:
        mats, lses, tg = R.case(V, ldl, P, L, bf, K)
        for tuples in R.tuple_sets(K):
            ref = R.reference(mats, lses, tg, P, V, tuples, float(R.B), R.offsets(K, off))
            nll, smp, ce = R.reference32(mats, lses, tg, P, V, tuples, float(R.B))
            for name, got, key, allow in (("nll", nll, "nll", "allow_nll"), ("sample_ce", smp, "sample_ce", "allow_sample"), ("ce", ce, "ce", "allow_ce")):
                err = (got.double() - ref[key]).abs()
                assert bool((err <= ref[allow]).all()), (name, K, tuples, float((err / ref[allow].clamp(min=1e-300)).max()))
            assert bool((ref["nll"][:, ~rows] == 0).all()) and bool(torch.isfinite(ref["nll"]).all())
            # the bound is a bound on fp32 work: a bf16 rounding of the guided scores would not fit (2^-9 of |g| against 2^-24)
            if V >= 255:
                assert float(ref["allow_nll"].max()) < 2.0 ** -9 * float(ref["nll"].abs().max())


@pytest.mark.parametrize("geo", [g for g in R.geometries() if g[0] in (9, 257, 4097)], ids=R.geo_id)
def test_two_matrices_are_the_guided_loss_reference(geo):
    """at K = 2 the rule is lu + s (lc - lu) up to float64 rounding: cfg_ref.reference on the same data, to 1e-12"""
    V, ldl, P, L, bf, off = geo
    mats, lses, tg = R.case(V, ldl, P, L, bf, 2)
    scales = [1.5, 0.0, 1.0, 7.5]
    ref = R.reference(mats, lses, tg, P, V, [(s,) for s in scales], float(R.B), R.offsets(2, off))
    old = cfg_ref.reference(mats[0], mats[1], lses[0], lses[1], tg, P, V, scales, float(R.B))
    for key in ("nll", "sample_ce", "ce"):
        assert bool(((ref[key] - old[key]).abs() <= 1e-12 * old[key].abs().clamp(min=1.0)).all()), key


def test_the_planted_cases_are_there():
    seen, paths = set(), set()
    for geo in R.geometries():
        V, ldl, P, L, bf, off = geo
        for K in R.KS:
            mats, lses, tg = R.case(V, ldl, P, L, bf, K)
            rows = cfg_ref.loss_rows(R.B, P, L)
            seen |= {int(x) - V for x in tg[:, 1:].reshape(-1) if x < 0 or x >= V}
            assert len(mats) == len(lses) == K and all(x.shape == (R.B * (P + L), ldl) and x.dtype == (torch.bfloat16 if bf else torch.float32) for x in mats)
            if V >= 2:
                for x in (mats[0], mats[K - 1]):
                    hi, lo = x[:, :V].float().max(1).values > 40, x[:, :V].float().min(1).values < -40
                    assert bool((hi & lo & rows).any())
            if ldl > V:
                assert all(float(x[:, V:].float().min()) > 9000 for x in mats)
            vec = R.vector_rows(R.B * (P + L), ldl, bf, R.offsets(K, off))
            paths |= {(geo[:2], bool(v)) for v in vec[rows]}
    assert {0, 5} <= seen and any(s < 0 for s in seen)       # V, V + 5 and a negative label
    assert (R.ODD, True) in paths and (R.ODD, False) in paths and (R.OFF, False) in paths and (R.OFF, True) not in paths and R.OFF[1] % 4 == 0
    for K in R.KS:
        one, mixed, eight = R.tuple_sets(K)
        assert len(one) == 1 and len(eight) == 8 and all(len(t) == K - 1 for ts in (one, mixed, eight) for t in ts)
        assert (0.0,) * (K - 1) in mixed and (1.0,) * (K - 1) in mixed and mixed[2] == mixed[4] and eight.count((1.0,) * (K - 1)) >= 2
        assert {0.0, 1.0, 7.5} <= {s for t in mixed for s in t}
