"""Distillation of a teacher's (guided) distribution, the part that needs no GPU: the float64 reference against itself, the new
entries in the header, the export map and the bindings, and every refusal that is made on the host."""
import ctypes
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cfg_ref as C
import kd_ref as R
from mmtg_amd import hip
from mmtg_amd.engine import Engine
from mmtg_amd.trainer import MMTGTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmtg_distill_fwd", "mmtg_loss_bwd_kd", "mmtg_loss_bwd_kd_x3")
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
SMALL = [g for g in R.geometries() if g[0] <= 257]


def _fwd(case, s, geo, exact_lse=False):
    V, ldl, ldt, P, L = geo
    x, lse, c, u, lse_c, lse_u, tg, topic, coef = case
    if exact_lse:
        lse = torch.logsumexp(x[:, :V].to(F64), 1)
    if s is None:
        return R.forward(x, lse, c, None, lse_c, None, 1.0, P, L, V, 2.0)
    return R.forward(x, lse, c, u, lse_c, lse_u, s, P, L, V, 2.0)


# ---- 1: the reference against itself
@pytest.mark.parametrize("geo", SMALL, ids=str)
def test_the_row_term_is_a_divergence(geo):
    V, ldl, ldt, P, L = geo
    case = R.case(V, ldl, ldt, P, L, False, False)
    rows = C.loss_rows(R.B, P, L)
    for s in R.SCALES:
        f = _fwd(case, s, geo, exact_lse=True)
        assert (f["kd_row"] >= -1e-12).all() and (f["kd_row"][~rows] == 0).all() and (f["kd_lg"][~rows] == 0).all()
        if V > 1:
            assert (f["kd_row"][rows] > 0).all()
        assert abs(float(f["kd_sample"].sum() / 2.0 - f["kd"])) <= 1e-12 * (1 + abs(float(f["kd"])))
        per = f["kd_row"].view(R.B, P + L)[:, P:P + L - 1].mean(1)
        assert torch.allclose(per, f["kd_sample"], rtol=1e-13, atol=1e-13)
        # the allowance is positive and small beside the magnitudes the row is formed from (|g| reaches hundreds at s = 7.5)
        size = 1 + f["g"].abs().max(1).values + f["logp"].abs().max(1).values
        assert (f["allow_row"][rows] > 0).all() and (f["allow_row"][rows] < 1e-4 * size[rows]).all()


@pytest.mark.parametrize("geo", SMALL, ids=str)
def test_a_teacher_equal_to_the_student_gives_zero(geo):
    V, ldl, ldt, P, L = geo
    x, lse, c, u, lse_c, lse_u, tg, topic, coef = R.case(V, ldl, ldt, P, L, False, False)
    lse64 = torch.logsumexp(x[:, :V].to(F64), 1)
    f = R.forward(x, lse64, x, None, lse64, None, 1.0, P, L, V, 2.0)
    assert abs(float(f["kd"])) <= 1e-12 and f["kd_row"].abs().max() <= 1e-12 and f["kd_lg"].abs().max() <= 1e-12
    # ... and with c == u the scale drops out
    a = R.forward(x, lse64, c, c, lse_c, lse_c, 0.0, P, L, V, 2.0)
    b = R.forward(x, lse64, c, c, lse_c, lse_c, 7.5, P, L, V, 2.0)
    assert torch.equal(a["kd_row"], b["kd_row"]) and torch.equal(a["kd"], b["kd"])


@pytest.mark.parametrize("geo", SMALL, ids=str)
def test_scale_one_with_a_negative_is_the_form_without(geo):
    V, ldl, ldt, P, L = geo
    case = R.case(V, ldl, ldt, P, L, False, False)
    a, b = _fwd(case, 1.0, geo), _fwd(case, None, geo)
    for k in ("kd_row", "kd_lg", "kd_sample", "kd"):
        assert torch.allclose(a[k], b[k], rtol=1e-12, atol=1e-12), k
    assert (a["allow_row"] >= b["allow_row"]).all()          # (the negative's operations are counted)


@pytest.mark.parametrize("s", [None, 0.0, 1.5, 7.5])
def test_the_gradient_is_the_objectives(s):
    V, P, L = 9, 3, 5
    x, lse, c, u, lse_c, lse_u, tg, topic, coef = R.case(V, 16, 16, P, L, False, False)
    x64 = x[:, :V].to(F64)
    lse64 = torch.logsumexp(x64, 1)
    uu, llu = (None, None) if s is None else (u, lse_u)
    f = R.forward(x64, lse64, c, uu, lse_c, llu, 1.0 if s is None else s, P, L, V, 2.0)
    d, allow = R.backward(x64, lse64, f, topic, tg, coef, R.GSCALE, R.LM_COEF, R.KD_COEF, P, V, 16)
    cf, active = R.row_factor(coef, R.GSCALE, R.LM_COEF, R.B, P, L)
    cf = torch.where(active, cf, torch.zeros_like(cf))
    lab = R.all_labels(topic, tg, P, V)
    w = float(np.float32(R.KD_COEF))
    obj = lambda z: R.objective(z, c, uu, lse_c, llu, 1.0 if s is None else s, cf, lab, f["rows"], w, V)
    h = 1e-5
    num = torch.zeros_like(x64)
    for m in range(x64.shape[0]):
        for v in range(V):
            e = torch.zeros_like(x64)
            e[m, v] = h
            num[m, v] = (obj(x64 + e) - obj(x64 - e)) / (2 * h)
    assert torch.allclose(num, d[:, :V], rtol=1e-6, atol=1e-8), float((num - d[:, :V]).abs().max())
    assert (d[:, V:] == 0).all() and (d[~active] == 0).all() and (allow[~active] == 0).all()
    # w = 0: the plain gradient, with a smaller allowance
    d0, allow0 = R.backward(x64, lse64, f, topic, tg, coef, R.GSCALE, R.LM_COEF, 0.0, P, V, 16)
    one = torch.zeros_like(x64)
    one[torch.arange(x64.shape[0]), lab] = 1.0
    assert torch.allclose(d0[:, :V], cf[:, None] * ((x64 - lse64[:, None]).exp() - one), rtol=1e-13, atol=1e-15)
    assert (allow0 <= allow).all()


# (bf16 rows are 16-byte aligned: the case of odd strides is fp32 on both sides)
STORED = [(g, sbf, tbf) for g in SMALL for (sbf, tbf) in ((False, False), (True, True), (False, True), (True, False))
          if g[1] % 8 == 0 or not (sbf or tbf)]


@pytest.mark.parametrize("geo,sbf,tbf", STORED, ids=str)
def test_a_float32_evaluation_is_inside_the_bounds(geo, sbf, tbf):
    """the rule evaluated in float32 by torch (its own order of summation) lies within the allowances: they are no underestimate of
    fp32 arithmetic.  (They were derived, not fitted: see kd_ref's docstring.)"""
    V, ldl, ldt, P, L = geo
    x, lse, c, u, lse_c, lse_u, tg, topic, coef = R.case(V, ldl, ldt, P, L, sbf, tbf)
    f32 = torch.float32
    for s in R.SCALES:
        f = _fwd((x, lse, c, u, lse_c, lse_u, tg, topic, coef), s, geo)
        lc = c[:, :V].to(f32) - lse_c[:, None]
        if s is None:
            g = lc
        else:
            lu = u[:, :V].to(f32) - lse_u[:, None]
            g = lu + torch.tensor(s, dtype=f32) * (lc - lu)
        logp = x[:, :V].to(f32) - lse[:, None]
        mx = g.max(1).values
        e = torch.exp(g - mx[:, None])
        S = e.sum(1)
        Lg = mx + S.log()
        row = (e * (g - logp)).sum(1) / S - Lg
        rows = f["rows"]
        assert ((row.to(F64) - f["kd_row"]).abs()[rows] <= f["allow_row"][rows]).all(), s
        assert ((Lg.to(F64) - f["kd_lg"]).abs()[rows] <= f["allow_lg"][rows]).all(), s
        d, allow = R.backward(x, lse, f, topic, tg, coef, R.GSCALE, R.LM_COEF, R.KD_COEF, P, V, R.padded(V))
        cf, active = R.row_factor(coef, R.GSCALE, R.LM_COEF, R.B, P, L)
        lab = R.all_labels(topic, tg, P, V)
        p = torch.exp(logp)
        one = torch.zeros_like(p)
        one[torch.arange(p.shape[0]), lab] = 1.0
        d32 = cf.float()[:, None] * (p - one) + torch.where(rows[:, None], torch.tensor(R.KD_COEF, dtype=f32) * (p - torch.exp(g - Lg[:, None])),
                                                          torch.zeros_like(p))
        d32 = torch.where(active[:, None], d32, torch.zeros_like(d32))
        assert ((d32.to(F64) - d[:, :V]).abs() <= allow[:, :V]).all(), s
        hi = d32.to(torch.bfloat16)
        assert ((hi.to(F64) - d[:, :V]).abs() <= R.allow_bf16(d, allow)[:, :V]).all(), s
        lo = (d32 - hi.float()).to(torch.bfloat16)
        assert (((hi.to(F64) + lo.to(F64)) - d[:, :V]).abs() <= R.allow_planes(d, allow)[:, :V]).all(), s


def test_the_cases_cover_the_kernel_paths():
    Vs = {g[0] for g in R.geometries()}
    assert set(C.VS) <= Vs and {2047, 2048, 2049, 2055, 2056, 2057} <= Vs
    assert R.geometries()[-1] == (255, 257, 259, 3, 5) and R.SCALES == [None, 0.0, 1.0, 1.5, 3.0, 7.5]
    x, lse, c, u, lse_c, lse_u, tg, topic, coef = R.case(160, 168, 168, 3, 5, True, False)
    assert x.dtype == torch.bfloat16 and c.dtype == torch.float32 and (x[:, 160:].float() > 9e3).all() and (coef[0] > 0 > coef[1])
    assert int(tg.max()) >= 160 and int(tg.min()) < 0 and int(topic.max()) >= 160


# ---- 2: the entries
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    exports = open(os.path.join(ROOT, "mmtg_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    lib = ctypes.CDLL(hip.lib_path())
    for name in ENTRIES:
        assert name + "(" in header and name in hip.exported_symbols() and name in hip._SIGS and hasattr(lib, name)
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), (name, patterns)
    assert [len(hip._SIGS[n][0]) for n in ENTRIES] == [21, 27, 26]
    assert hip.lib().mmtg_abi_version() == hip.ABI_VERSION == 12 and "#define MMTG_ABI_VERSION 12" in header
    assert callable(hip.distill_fwd) and callable(hip.loss_bwd_kd) and callable(hip.loss_bwd_kd_x3)
    assert os.path.exists(os.path.join(ROOT, "mmtg_amd", "csrc", "distill.hip"))
    for name, args in (("distill_loss", ("teacher_logits", "teacher_lse", "uncond_logits", "uncond_lse", "scale", "batch_den")),
                       ("loss_backward_kd", ("gscale", "lm_coef", "kd_coef"))):
        assert tuple(inspect.signature(getattr(Engine, name)).parameters)[1:] == args
    sig = inspect.signature(MMTGTrainer.__init__).parameters
    assert sig["distill_weight"].default == 0.0 and sig["distill_teacher"].default is None and sig["distill_scale"].default == 1.0


# ---- 3: fake device addresses: every case is refused on the host, before any device call, so no GPU is touched
A = [0x7000000000 + 0x100000000 * i for i in range(16)]


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


def test_distill_fwd_checks_its_arguments():
    #       ldt x    ldl  tdt cond  uncond ldt  V    lse   lse_c lse_u s    B  P  L  den  row   lg    smp   kd     stream
    good = [1, A[0], 168, 1, A[1], A[2], 168, 160, A[3], A[4], A[5], 2.0, 2, 3, 5, 2.0, A[6], A[7], A[8], A[9], None]
    M = 2 * 8
    bad = {"dtype": (0, 5, "dtype"), "teacher dtype": (3, 9, "teacher dtype"), "null logits": (1, None, "logits"),
           "null cond": (4, None, "cond"), "null uncond alone": (5, None, "null together"), "null lse_u alone": (10, None, "null together"),
           "null lse": (8, None, "lse"), "null lse_c": (9, None, "lse_c"), "null kd_row": (16, None, "kd_row"), "null kd_lg": (17, None, "kd_lg"),
           "null kd_sample": (18, None, "kd_sample"), "null kd": (19, None, "kd is"),
           "scale nan": (11, NAN, "scale"), "scale inf": (11, INF, "scale"), "scale < 0": (11, -0.5, "scale"),
           "V = 0": (7, 0, "V ="), "V < 0": (7, -4, "V ="), "ldl < V": (2, 152, "ldl"), "ldt < V": (6, 152, "ldt"),
           "bf16 ldl % 8": (2, 164, "bf16 rows"), "bf16 ldt % 8": (6, 164, "bf16 teacher rows"),
           "misaligned bf16 logits": (1, A[0] + 2, "bf16 rows"), "misaligned bf16 cond": (4, A[1] + 2, "bf16 teacher rows"),
           "misaligned bf16 uncond": (5, A[2] + 8, "bf16 teacher rows"), "misaligned f32 logits": ((0, 1), (0, A[0] + 2), "fp32 rows"),
           "misaligned f32 cond": ((3, 4), (0, A[1] + 2), "fp32 teacher rows"),
           "B = 0": (12, 0, "B ="), "P < 0": (13, -1, "P ="), "L = 1": (14, 1, "L ="), "L = 0": (14, 0, "L ="),
           "batch_den 0": (15, 0.0, "batch_den"), "batch_den < 0": (15, -2.0, "batch_den"), "batch_den nan": (15, NAN, "batch_den"),
           "batch_den inf": (15, INF, "batch_den"),
           "kd_row is cond": (16, A[1], "overlaps"), "kd_lg ends in uncond": (17, A[2] - 4 * M + 4, "overlaps"),
           "kd_sample in lse_c": (18, A[4] + 8, "overlaps"), "kd is the last of lse_u": (19, A[5] + 4 * (M - 1), "overlaps"),
           "kd_row in cond's last row": (16, A[1] + 2 * ((M - 1) * 168 + 159), "overlaps")}
    _each(hip.lib().mmtg_distill_fwd, "distill_fwd", good, bad)
    # without a negative the scale is still checked, and an output may lie where the negative would have been
    none = list(good)
    none[5], none[10], none[16], none[14] = None, None, A[2], 1
    _refused(hip.lib().mmtg_distill_fwd, "distill_fwd", none, "L is what is refused", "L =")


def _bwd_cases(o):
    """what both backward entries refuse alike; o: index of the first teacher argument"""
    return {"null cond": (o + 1, None, "cond"), "null uncond alone": (o + 2, None, "null together"), "null lse_u alone": (o + 5, None, "null together"),
            "null lse_c": (o + 4, None, "lse_c"), "null kd_lg": (o + 7, None, "kd_lg"), "teacher dtype": (o, 7, "teacher dtype"),
            "scale nan": (o + 6, NAN, "scale"), "scale inf": (o + 6, INF, "scale"), "scale < 0": (o + 6, -1.0, "scale"),
            "ldt < V": (o + 3, 152, "ldt"), "bf16 ldt % 8": (o + 3, 164, "bf16 teacher rows"),
            "misaligned bf16 cond": (o + 1, A[4] + 2, "bf16 teacher rows"),
            "kd_coef nan": (o + 8, NAN, "kd_coef"), "kd_coef inf": (o + 8, INF, "kd_coef"), "kd_coef < 0": (o + 8, -0.1, "kd_coef"),
            "B = 0": (o + 9, 0, "B ="), "P < 0": (o + 10, -1, "P ="), "L = 1": (o + 11, 1, "L =")}


def test_loss_bwd_kd_checks_its_arguments():
    #       dt lt x    ldl  V    topic targets lse  coef  gs   lm   tdt cond  uncond ldt  lse_c lse_u s    kd_lg kdc  B  P  L  dlogits ldd Vpad stream
    good = [1, 1, A[0], 168, 160, A[1], A[2], A[3], A[10], 2.0, 0.0, 1, A[4], A[5], 168, A[6], A[7], 2.0, A[8], 0.5, 2, 3, 5, A[9], 168, 160, None]
    M = 2 * 8
    bad = dict(_bwd_cases(11))
    bad.update({"dtype": (0, 5, "dtype"), "f32 dlogits of bf16 logits": (0, 0, "bf16 logits go with"), "null logits": (2, None, "logits"),
                "null targets": (6, None, "targets"), "null lse": (7, None, "lse"), "null coef": (8, None, "coef"),
                "null dlogits": (23, None, "dlogits"), "null topic_ids with lm_coef": ((5, 10), (None, 0.5), "topic_ids"),
                "V = 0": (4, 0, "V ="), "ldl < V": (3, 152, "ldl"), "Vpad < V": (25, 152, "Vpad"), "ldd < Vpad": (24, 152, "Vpad"),
                "bf16 ldl % 8": (3, 164, "bf16 rows"), "misaligned bf16 logits": (2, A[0] + 2, "bf16 rows"),
                "in-place with another stride": ((23, 24), (A[0], 176), "in-place"),
                "dlogits is cond": (23, A[4], "overlaps"), "dlogits ends in uncond": (23, A[5] - 2, "overlaps"),
                "dlogits begins in cond's last row": (23, A[4] + 2 * ((M - 1) * 168 + 159), "overlaps"),
                "dlogits over lse_c": (23, A[6] - 16, "overlaps"), "dlogits over kd_lg": (23, A[8] + 4 * (M - 1), "overlaps")})
    _each(hip.lib().mmtg_loss_bwd_kd, "loss_bwd_kd", good, bad)
    inplace = list(good)
    inplace[23], inplace[22] = A[0], 1                      # the in-place bf16 form is not what is refused
    _refused(hip.lib().mmtg_loss_bwd_kd, "loss_bwd_kd", inplace, "L is what is refused", "L =")


def test_loss_bwd_kd_x3_checks_its_arguments():
    M = 2 * 8
    plane = M * 160
    #       x    ldl  V    topic targets lse  coef  gs   lm   tdt cond  uncond ldt  lse_c lse_u s    kd_lg kdc  B  P  L  planes ldd plane Vpad stream
    good = [A[0], 160, 160, A[1], A[2], A[3], A[10], 2.0, 0.0, 0, A[4], A[5], 161, A[6], A[7], 2.0, A[8], 0.5, 2, 3, 5, A[9], 160, plane, 160, None]
    bad = dict(_bwd_cases(9))
    del bad["bf16 ldt % 8"], bad["misaligned bf16 cond"]                # (this teacher is fp32, of an odd stride)
    bad.update({"null logits": (0, None, "logits"), "null planes": (21, None, "dlogits"), "plane = 0": (23, 0, "plane"),
                "ldl % 4": (1, 162, "ldl"), "ldl < Vpad": ((1, 2), (152, 150), "ldl"), "misaligned logits": (0, A[0] + 4, "ldl"),
                "Vpad % 8": ((24, 2), (156, 150), "multiples of 8"), "ldd % 8": (22, 164, "multiples of 8"),
                "misaligned planes": (21, A[9] + 8, "multiples of 8"), "lo plane inside hi": (23, plane - 8, "lo plane"),
                "bf16 teacher ldt % 8": ((9, 12), (1, 164), "bf16 teacher rows"),
                "lo plane over cond": (21, A[4] - 2 * plane, "overlaps"), "planes are uncond": (21, A[5], "overlaps")})
    _each(hip.lib().mmtg_loss_bwd_kd_x3, "loss_bwd_kd_x3", good, bad)


def test_the_bindings_refuse_a_half_given_negative():
    t = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="together"):
        hip._teacher(t, t, None)
    with pytest.raises(ValueError, match="together"):
        hip._teacher(t, None, t[:, 0])
    with pytest.raises(ValueError, match="one storage type"):
        hip._teacher(t, t.bfloat16(), t[:, 0])


# ---- 4: the trainer's refusals
class _Model:
    """what MMTGTrainer's constructor touches"""
    training = True

    class _Layout:
        total = 4

    class _Sh:
        def __init__(self, V, P):
            self.V, self.P = V, P

    class _Eng:
        dev = torch.device("cpu")
        opt_m = opt_v = ema = None
        step_count, drop_seed = 0, 1

    def __init__(self, V=160, P=3):
        self._eng = self._Eng()
        self._eng.layout = self._Layout()
        self._eng.sh = self._Sh(V, P)

    def engine(self):
        return self._eng


def test_the_trainer_refuses_what_the_term_cannot_do():
    student, teacher = _Model(), _Model()
    with pytest.raises(ValueError, match="needs distill_teacher"):
        MMTGTrainer(student, distill_weight=0.5)
    with pytest.raises(ValueError, match="distill_weight = 0"):
        MMTGTrainer(student, distill_teacher=teacher)
    with pytest.raises(ValueError, match="ul_weight"):
        MMTGTrainer(student, distill_weight=0.5, distill_teacher=teacher, ul_weight=0.1)
    with pytest.raises(ValueError, match="experience_drop"):
        MMTGTrainer(student, distill_weight=0.5, distill_teacher=teacher, experience_drop=0.1)
    with pytest.raises(ValueError, match="pass a copy"):
        MMTGTrainer(student, distill_weight=0.5, distill_teacher=student)
    shared = _Model()
    shared._eng = student._eng
    with pytest.raises(ValueError, match="pass a copy"):
        MMTGTrainer(student, distill_weight=0.5, distill_teacher=shared)
    with pytest.raises(ValueError, match="V = 161"):
        MMTGTrainer(student, distill_weight=0.5, distill_teacher=_Model(V=161))
    with pytest.raises(ValueError, match="P = 4"):
        MMTGTrainer(student, distill_weight=0.5, distill_teacher=_Model(P=4))
    for bad in (-0.5, NAN, INF, "1", True, None):
        with pytest.raises(ValueError, match="distill_weight"):
            MMTGTrainer(None, distill_weight=bad)
        with pytest.raises(ValueError, match="distill_scale"):
            MMTGTrainer(None, distill_scale=bad)


def test_the_arguments_are_recorded_and_the_teacher_is_not():
    student, teacher = _Model(), _Model()
    tr = MMTGTrainer(student, distill_weight=0.5, distill_teacher=teacher, distill_scale=2)
    assert tr.distill_weight == 0.5 and tr.distill_scale == 2.0 and type(tr.distill_scale) is float and tr.teng is teacher.engine()
    sd = tr.state_dict()
    assert sd["hparams"]["distill_weight"] == 0.5 and sd["hparams"]["distill_scale"] == 2.0
    assert not any("teacher" in k for k in sd) and not any("teacher" in k for k in sd["hparams"])
    plain = MMTGTrainer(_Model())
    assert plain.distill_weight == 0.0 and plain.teng is None and plain.state_dict()["hparams"]["distill_weight"] == 0.0
    plain.load_state_dict(sd)
    assert plain.distill_weight == 0.0                               # the trainer's own stays
    old = dict(sd, hparams={k: v for k, v in sd["hparams"].items() if not k.startswith("distill_")})
    tr.load_state_dict(old)                                          # a checkpoint from before the option loads
    assert tr.distill_weight == 0.5
