"""The training side of guidance, the host side: the two entries' declarations and argument checks, the numpy restatement of the code
rule of mmtg_experience_drop, the trainer's arguments, and a float32 evaluation of mmtg_guided_loss's expressions inside the bounds
of tests/cfg_ref.py on every case of tests/test_cfg_ops_gpu.py.  No GPU."""
import ctypes
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cfg_ref as R
from mmtg_amd import engine, hip
from mmtg_amd.trainer import MMTGTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmtg_experience_drop", "mmtg_guided_loss")


# ---- 1
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    exports = open(os.path.join(ROOT, "mmtg_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    lib = ctypes.CDLL(hip.lib_path())
    for name in ENTRIES:
        assert name + "(" in header and name in hip.exported_symbols() and name in hip._SIGS and hasattr(lib, name)
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), (name, patterns)
    assert [len(hip._SIGS[n][0]) for n in ENTRIES] == [13, 19]
    assert hip.lib().mmtg_abi_version() == hip.ABI_VERSION == 12
    assert "#define MMTG_ABI_VERSION 12" in header and "MMTG_GUIDED_MAX_SCALES 8" in header
    assert callable(hip.experience_drop) and callable(hip.guided_loss) and hip.GUIDED_MAX_SCALES == 8
    assert os.path.exists(os.path.join(ROOT, "mmtg_amd", "csrc", "guidance_train.hip"))
    assert engine.EXP_DROP_SITE == R.EXP_DROP_SITE and engine.mix_seed(12345, 7) == R.mix_seed(12345, 7)


# ---- 2: fake device addresses: every case is refused on the host, before any device call, so no GPU is touched
A = [0x7000000000 + 0x100000000 * i for i in range(10)]
NAN, INF = float("nan"), float("inf")
T32 = 1 << 32


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


def test_experience_drop_checks_its_arguments():
    #       dtype img  txt   img_out txt_out code  B  n   seed c_both c_img c_txt stream
    good = [1, A[0], A[1], A[2], A[3], A[4], 4, 64, 7, 100, 200, 300, None]
    bad = {"dtype": (0, 7, "dtype"), "null img": (1, None, "img"), "null txt": (2, None, "txt"), "null img_out": (3, None, "img_out"),
           "null txt_out": (4, None, "txt_out"), "null code": (5, None, "code"), "B = 0": (6, 0, "B ="), "B < 0": (6, -3, "B ="),
           "n = 0": (7, 0, "n ="), "n < 0": (7, -8, "n ="), "c_both > c_img": (9, 201, "thresholds"), "c_img > c_txt": (10, 301, "thresholds"),
           "c_txt > 2^32": (11, T32 + 1, "thresholds"), "c_both < 0": (9, -1, "thresholds"),
           "all above 2^32": ((9, 10, 11), (T32 + 1, T32 + 2, T32 + 3), "thresholds"),
           "img_out is img": (3, A[0], "img_out overlaps"), "img_out inside txt": (3, A[1] + 4 * 100, "img_out overlaps"),
           "txt_out is txt": (4, A[1], "txt_out overlaps"), "txt_out ends in img": (4, A[0] - 2, "txt_out overlaps"),
           "f32 img_out ends in img": ((0, 3), (0, A[0] - 4), "img_out overlaps")}
    _each(hip.lib().mmtg_experience_drop, "experience_drop", good, bad)


def test_guided_loss_checks_its_arguments():
    sc = (ctypes.c_float * 8)(0.0, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 7.5)
    S = ctypes.addressof(sc)
    arr = lambda *v: ctypes.addressof(_keep.setdefault(v, (ctypes.c_float * 8)(*(v + (1.0,) * (8 - len(v))))))
    #       ldt cond  uncond ldl V    lse_c lse_u topic targets scales K B P L  den  nll   smp   ce   stream
    good = [1, A[0], A[1], 168, 160, A[2], A[3], A[4], A[5], S, 8, 2, 3, 5, 2.0, A[6], A[7], A[8], None]
    bad = {"dtype": (0, 5, "dtype"), "null cond": (1, None, "cond"), "null uncond": (2, None, "uncond"), "null lse_c": (5, None, "lse_c"),
           "null lse_u": (6, None, "lse_u"), "null targets": (8, None, "targets"), "null scales": (9, None, "scales"),
           "null nll": (15, None, "nll"), "null sample_ce": (16, None, "sample_ce"), "null ce": (17, None, "ce"),
           "K = 0": (10, 0, "K ="), "K = 9": (10, 9, "K ="), "K < 0": (10, -1, "K ="),
           "scale nan": (9, arr(1.0, NAN), "scale 1"), "scale inf": (9, arr(INF), "scale 0"), "scale < 0": (9, arr(1.0, 2.0, -0.5), "scale 2"),
           "V = 0": (4, 0, "V ="), "V < 0": (4, -4, "V ="), "ldl < V": (3, 152, "ldl"), "bf16 ldl % 8": (3, 164, "bf16 rows"),
           "misaligned bf16 cond": (1, A[0] + 2, "bf16 rows"), "misaligned bf16 uncond": (2, A[1] + 8, "bf16 rows"),
           "misaligned f32 cond": ((0, 1), (0, A[0] + 2), "fp32 rows"),
           "B = 0": (11, 0, "B ="), "P < 0": (12, -1, "P ="), "L = 1": (13, 1, "L ="), "L = 0": (13, 0, "L ="),
           "batch_den 0": (14, 0.0, "batch_den"), "batch_den < 0": (14, -2.0, "batch_den"), "batch_den nan": (14, NAN, "batch_den"),
           "batch_den inf": (14, INF, "batch_den")}
    _each(hip.lib().mmtg_guided_loss, "guided_loss", good, bad)
    # a scale behind the K that are read is not looked at; topic_ids is never read and may be null
    ok = list(good)
    ok[9], ok[10] = arr(1.0, NAN), 1
    bad_after = list(ok)
    bad_after[13] = 1
    _refused(hip.lib().mmtg_guided_loss, "guided_loss", bad_after, "K = 1 beside a NaN in slot 1: L is what is refused", "L =")
    no_topic = list(good)
    no_topic[7], no_topic[13] = None, 1
    _refused(hip.lib().mmtg_guided_loss, "guided_loss", no_topic, "null topic_ids is not what is refused", "L =")


_keep = {}


# ---- 3: the code rule, restated in numpy
def test_the_threshold_formula_and_the_code_rule():
    assert R.thresholds((0.0, 0.0, 0.0)) == (0, 0, 0) and R.thresholds((1.0, 0.0, 0.0)) == (T32, T32, T32)
    assert R.thresholds((0.0, 1.0, 0.0)) == (0, T32, T32) and R.thresholds((0.0, 0.0, 1.0)) == (0, 0, T32)
    assert R.thresholds(R.MIXED) == (int(0.25 * 2.0 ** 32), int(0.25 * 2.0 ** 32) + int(0.10 * 2.0 ** 32),
                                     int(0.25 * 2.0 ** 32) + int(0.10 * 2.0 ** 32) + int(0.15 * 2.0 ** 32))
    for probs in ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), R.MIXED, (0.3, 0.2, 0.2), (0.5, 0.5, 0.0)):
        assert hip.drop_thresholds(probs) == R.thresholds(probs)
    for seed in R.KERNEL_SEEDS:
        assert not R.codes(seed, 4096, (0, 0, 0)).any() and bool((R.codes(seed, 4096, (T32, T32, T32)) == 3).all())
        assert bool((R.codes(seed, 4096, (0, T32, T32)) == 1).all()) and bool((R.codes(seed, 4096, (0, 0, T32)) == 2).all())
    # the hash is the one of csrc/common.h (a value computed by hand from its five lines)
    h = 5 * 0x9E3779B1 + 77 & 0xFFFFFFFF
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    h ^= h >> 16
    assert int(R.hash_u32(77, np.arange(6))[5]) == h


@pytest.mark.parametrize("seed", R.KERNEL_SEEDS)
def test_the_three_counts_are_binomial(seed):
    n = 65536
    cd = R.codes(seed, n, R.thresholds(R.MIXED))
    for code, p in ((3, 0.25), (1, 0.10), (2, 0.15)):
        z = (int((cd == code).sum()) - n * p) / np.sqrt(n * p * (1 - p))
        assert abs(z) <= 5.0, (seed, code, z)
    assert int((cd == 0).sum()) + int((cd != 0).sum()) == n and set(np.unique(cd)) <= {0, 1, 2, 3}


# ---- 4: the trainer's arguments (refused before the model is touched)
@pytest.mark.parametrize("value", [-0.1, 1.5, NAN, INF, "0.5", True, None, (0.5, 0.5, 0.5), (0.1, 0.2), (0.1, 0.2, 0.3, 0.1), (0.1, 0.2, "a"),
                                   (0.1, True, 0.1), (0.1, -0.2, 0.3), (0.1, NAN, 0.1), (1.5, 0.0, 0.0), {"p": 0.1}, b"0.1"])
def test_the_trainer_refuses_a_malformed_experience_drop(value):
    with pytest.raises(ValueError, match="experience_drop"):
        MMTGTrainer(None, experience_drop=value)


class _Model:
    """what MMTGTrainer's constructor touches"""
    training = True

    class _Layout:
        total = 4

    class _Eng:
        dev = torch.device("cpu")
        opt_m = opt_v = ema = None
        step_count, drop_seed = 0, 1

    def __init__(self):
        self._eng = self._Eng()
        self._eng.layout = self._Layout()

    def engine(self):
        return self._eng


def test_normalisation_and_the_hparams_round_trip():
    from mmtg_amd.trainer import _check_experience_drop as norm
    assert norm(0.0) == (0.0, 0.0, 0.0) and norm(0) == (0.0, 0.0, 0.0) and norm(1) == (1.0, 0.0, 0.0) and norm(0.1) == (0.1, 0.0, 0.0)
    assert norm([0.25, 0.10, 0.15]) == (0.25, 0.10, 0.15) and norm((0.5, 0.5, 0.0)) == (0.5, 0.5, 0.0)
    assert norm(np.float64(0.2)) == (0.2, 0.0, 0.0) and all(type(v) is float for v in norm(np.float64(0.2)))
    assert "experience_drop" in inspect.signature(MMTGTrainer.__init__).parameters
    assert inspect.signature(MMTGTrainer.__init__).parameters["experience_drop"].default == 0.0
    tr = MMTGTrainer(_Model(), experience_drop=(0.3, 0.2, 0.2))
    assert tr.experience_drop == (0.3, 0.2, 0.2) and tr._exp_drop_on
    assert MMTGTrainer(_Model()).experience_drop == (0.0, 0.0, 0.0) and not MMTGTrainer(_Model(), experience_drop=0.0)._exp_drop_on
    sd = tr.state_dict()
    assert sd["hparams"]["experience_drop"] == (0.3, 0.2, 0.2)
    assert MMTGTrainer(_Model(), experience_drop=0.25).state_dict()["hparams"]["experience_drop"] == (0.25, 0.0, 0.0)
    other = MMTGTrainer(_Model(), experience_drop=0.1)
    other.load_state_dict(sd)
    assert other.experience_drop == (0.1, 0.0, 0.0)                 # the trainer's own stays
    old = dict(sd, hparams={k: v for k, v in sd["hparams"].items() if k != "experience_drop"})
    other.load_state_dict(old)                                      # a checkpoint from before the option loads
    assert other.experience_drop == (0.1, 0.0, 0.0) and other.eng.drop_seed == sd["drop_seed"]


def test_scales_are_refused_as_check_guidance_refuses_them():
    tr = MMTGTrainer.__new__(MMTGTrainer)           # the scales are checked before anything of the trainer is touched
    for fn in (lambda s: tr.evaluate_guided_batch({}, s), lambda s: tr.evaluate_guided([], s)):
        for bad in ([], [1.0] * 9, [NAN], [1.0, -0.5], [INF], ["2"], [True], [None], "12", 3.0, None):
            with pytest.raises(ValueError, match="scale"):
                fn(bad)
    for name in ("evaluate_guided_batch", "evaluate_guided"):
        assert "scales" in inspect.signature(getattr(MMTGTrainer, name)).parameters
    for name in ("evaluate_batch", "evaluate"):
        assert inspect.signature(getattr(MMTGTrainer, name)).parameters["without_experience"].default is False


# ---- 5: the kernel's expressions in float32 stay inside the bounds, on every case of the GPU file
@pytest.mark.parametrize("geo", R.geometries(), ids=lambda g: "V%d-ld%d-P%d-L%d-%s" % (g[:4] + ("bf16" if g[4] else "f32",)))
def test_a_float32_evaluation_is_inside_the_bounds(geo):
    V, ldl, P, L, bf = geo
    c, u, lse_c, lse_u, tg = R.case(*geo)
    for scales in R.KSETS:
        ref = R.reference(c, u, lse_c, lse_u, tg, P, V, scales, float(R.B))
        nll, smp, ce = R.reference32(c, u, lse_c, lse_u, tg, P, V, scales, float(R.B))
        for name, got, key, allow in (("nll", nll, "nll", "allow_nll"), ("sample_ce", smp, "sample_ce", "allow_sample"), ("ce", ce, "ce", "allow_ce")):
            err = (got.double() - ref[key]).abs()
            assert bool((err <= ref[allow]).all()), (name, scales, float((err / ref[allow].clamp(min=1e-300)).max()))
        rows = R.loss_rows(R.B, P, L)
        assert bool((ref["nll"][:, ~rows] == 0).all()) and bool((ref["nll"][:, rows] >= 0).all())
        # the bound is a bound on fp32 work: a bf16 rounding of the guided scores would not fit (2^-9 of |g| against 2^-24)
        if V >= 160:
            assert float(ref["allow_nll"].max()) < 2.0 ** -9 * float(ref["nll"].max())


def test_the_planted_cases_are_there():
    seen = set()
    for geo in R.geometries():
        V, ldl, P, L, bf = geo
        c, u, lse_c, lse_u, tg = R.case(*geo)
        labels = tg[:, 1:]
        seen |= {int(x) - V for x in labels.reshape(-1) if x < 0 or x >= V}
        assert c.shape == (R.B * (P + L), ldl) and c.dtype == (torch.bfloat16 if bf else torch.float32)
        if V >= 2:
            assert float(c[:, :V].float().max()) > 40 and float(c[:, :V].float().min()) < -40
        if ldl > V:
            assert float(c[:, V:].float().min()) > 9000
    assert {0, 5} <= seen and any(s < 0 for s in seen)       # V, V + 5 and a negative label
    assert (R.ODD[0], R.ODD[1], 3, 5, False) in R.geometries() and R.ODD[1] % 2 == 1
