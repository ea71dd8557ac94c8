"""MMTGTrainer(distill_weight=..., distill_teacher=..., distill_scale=...) on the real engine: the tiny 2-layer model with tiny_s5's
weights (V = 160, P = 15, L = 221) as student and as teacher, synthetic batches, all four compute modes.  The kernels alone are in
tests/test_kd_ops_gpu.py, the host side in tests/test_kd_cpu.py; the reference and its bounds in tests/kd_ref.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kd_ref as R  # noqa: E402
from helpers import load_case  # noqa: E402
from mmtg_amd import MMTG, hip, synth  # noqa: E402
from mmtg_amd.trainer import MMTGTrainer  # noqa: E402

DEV = "cuda"
# student mode, teacher mode: every student mode once, the teacher in three storage / mode combinations
PAIRS = [("bf16", "bf16"), ("f32", "bf16"), ("bf16x3", "f32"), ("bf16x3f", "bf16x3")]


@functools.lru_cache(maxsize=None)
def _case():
    fx, meta, mcfg, gcfg, dcfg, weights, table, _ = load_case("tiny_s5")
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    return meta, mcfg, gcfg, dcfg, sd, table


def build(mode, pdrop=0.0, shift=0.0):
    """shift: the teacher's weights moved off the student's by that much noise (a seeded draw), so that the two distributions differ"""
    meta, mcfg, gcfg, dcfg, sd, table = _case()
    gcfg = dict(gcfg, embd_pdrop=pdrop, attn_pdrop=pdrop, resid_pdrop=pdrop)
    model = MMTG(mcfg, dcfg, meta["V"], train_flag=True, gpt2_config=gcfg, token_table=table, compute_dtype=mode)
    if shift:
        gen = torch.Generator().manual_seed(99)
        sd = {k: v + shift * torch.randn(v.shape, generator=gen).to(v.dtype) if v.is_floating_point() else v for k, v in sd.items()}
    model.load_state_dict(sd)
    model.to(DEV)
    model.train(pdrop > 0)
    return model


@functools.lru_cache(maxsize=None)
def rows(n, seed=7):
    meta, mcfg, gcfg, dcfg, sd, table = _case()
    nb = synth.make_batch(n, mcfg, dcfg, meta["V"], seed=seed)
    return {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nb.items()}


def part(lo, hi, n=5):
    return {k: v[lo:hi] for k, v in rows(n).items()}


def _within(name, got, ref, allow):
    err = (got.double() - ref).abs()
    assert bool((err <= allow).all()), "%s: %d outside the bound, worst err/allowed %.3g" % (
        name, int((err > allow).sum()), float((err / allow.clamp(min=1e-300)).max()))


def _engine_pass(tr, batch, n):
    """the trainer's micro-step up to the term's forward, on the engine; returns the CPU copies the reference reads"""
    eng = tr.eng
    teacher = tr._teacher_pass(batch, 3)
    eng.forward(batch, train_flag=True, training=False, logits_f32=False)
    eng.loss(batch["rating"], 3, batch_den=n)
    kd = eng.distill_loss(*teacher, scale=tr.distill_scale, batch_den=n)
    a = eng.act
    host = dict(x=a["logits"].detach().cpu().clone(), lse=a["lse_rows"].cpu(), tg=a["targets"].cpu(), topic=a["topic_ids"].cpu(),
                coef=a["coef"].cpu(), c=teacher[0].cpu(), lse_c=teacher[1].cpu(), u=None if teacher[2] is None else teacher[2].cpu(),
                lse_u=None if teacher[3] is None else teacher[3].cpu())
    return kd, host


# ---- 1
@pytest.mark.parametrize("scale", [2.0, 1.0])
@pytest.mark.parametrize("mode,tmode", PAIRS)
def test_the_engine_follows_the_rule_on_its_own_logits(mode, tmode, scale):
    """kd, the rows, Lg and d(logits) of the engine against kd_ref on the logits the student's and the teacher's engines themselves
    produced (bf16: read back before the backward overwrites them); step() returns the same 'kd' bits"""
    w, n = 0.5, 5
    batch = part(0, n)
    teacher = build(tmode, shift=0.02)
    tr = MMTGTrainer(build(mode), lr=0.0, alpha=0.2, distill_weight=w, distill_teacher=teacher, distill_scale=scale)
    eng, sh = tr.eng, tr.eng.sh
    kd, h = _engine_pass(tr, batch, n)
    a = eng.act
    V, P, L, Vp = sh.V, sh.P, a["L"], eng.layout.Vpad
    assert h["x"].dtype == (torch.bfloat16 if mode == "bf16" else torch.float32) and h["x"].shape == (n * (P + L), Vp)
    assert h["c"].dtype == (torch.bfloat16 if tmode == "bf16" else torch.float32) and (h["u"] is None) == (scale == 1.0)
    fw = R.forward(h["x"], h["lse"], h["c"], h["u"], h["lse_c"], h["lse_u"], scale, P, L, V, float(n))
    print(mode, tmode, scale, "kd %.6f ref %.6f" % (float(kd), float(fw["kd"])))
    assert float(fw["kd"]) > 1e-3                                              # the teacher does differ
    _within("kd_row", a["kd_row"].cpu(), fw["kd_row"], fw["allow_row"])
    _within("kd_lg", a["kd_lg"].cpu(), fw["kd_lg"], fw["allow_lg"])
    _within("kd_sample", a["kd_sample"].cpu(), fw["kd_sample"], fw["allow_sample"])
    _within("kd", kd.cpu(), fw["kd"].reshape(1), fw["allow_kd"].reshape(1))
    kd_bits = kd.cpu().clone()
    wc = w / ((L - 1) * n) * float(n)
    dl = eng.loss_backward_kd(float(n), 0.0, wc)
    d, allow = R.backward(h["x"], h["lse"], fw, h["topic"], h["tg"], h["coef"], float(n), 0.0, wc, P, V, Vp)
    if mode == "bf16x3":
        _within("d(logits)", dl.float().cpu(), d, R.allow_planes(d, allow))
    else:
        assert (dl.data_ptr() == a["logits"].data_ptr()) == (mode == "bf16")   # bf16: the logits are rewritten in place
        assert dl.dtype == (torch.float32 if mode == "f32" else torch.bfloat16)
        _within("d(logits)", dl.cpu(), d, allow if mode == "f32" else R.allow_bf16(d, allow))
    d0, _ = R.backward(h["x"], h["lse"], fw, h["topic"], h["tg"], h["coef"], float(n), 0.0, 0.0, P, V, Vp)
    assert float((d - d0).abs().sum()) > 0.1 * float(d0.abs().sum()), "the term hardly changes d(logits)"
    out = tr.step(batch, stage=3)
    assert torch.equal(out["kd"].cpu().reshape(1).view(torch.int32), kd_bits.view(torch.int32))
    assert sorted(out) == ["kd", "kl", "lm_loss", "loss"] and float(tr.window["kd"]) == float(out["kd"])
    assert bool(torch.isfinite(out["kd"])) and float(out["kd"]) >= 0
    ev = tr.evaluate_batch(batch)
    assert float(ev["kd"]) == float(kd_bits) and float(ev["total"]) == pytest.approx(float(ev["loss"]) + 0.2 * float(ev["kl"]), rel=1e-6)


# ---- 2
@pytest.mark.parametrize("mode", ["bf16", "f32", "bf16x3", "bf16x3f"])
def test_a_copy_of_the_student_teaches_nothing(mode):
    """the teacher holds the student's weights, both in eval mode, scale 1: the two logits matrices are the same bits and kd is
    what the reference allows for identical logits (the fp32 lse is not the exact one, so the reference's own value is not 0)"""
    n = 5
    batch = part(0, n)
    tr = MMTGTrainer(build(mode), lr=0.0, alpha=0.2, distill_weight=1.0, distill_teacher=build(mode))
    kd, h = _engine_pass(tr, batch, n)
    assert torch.equal(h["x"], h["c"]) and torch.equal(h["lse"], h["lse_c"]) and h["u"] is None
    sh = tr.eng.sh
    fw = R.forward(h["x"], h["lse"], h["c"], None, h["lse_c"], None, 1.0, sh.P, tr.eng.act["L"], sh.V, float(n))
    print(mode, "kd %.3e, reference %.3e, allowed %.3e" % (float(kd), float(fw["kd"]), float(fw["allow_kd"])))
    assert abs(float(kd)) <= float(fw["allow_kd"]) + abs(float(fw["kd"]))
    assert float(fw["allow_kd"]) < 1e-4


# ---- 3
def _launches(tr, batch):
    hip.prof_enable(True)
    try:
        tr.step(batch, stage=3)
        rec = hip.prof_read()
    finally:
        hip.prof_enable(False)
    return {k: v["launches"] for k, v in rec.items()}


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_the_default_is_today_s_trainer(mode):
    """distill_weight=0.0 against the keywords left out: equal launch counts per step in every category of the library's profiler,
    and after two steps with dropout on equal bits in the parameters and both moments; no buffer of the term exists"""
    trs = []
    for kw in ({"distill_weight": 0.0, "distill_teacher": None, "distill_scale": 1.0}, {}):
        tr = MMTGTrainer(build(mode, 0.1), lr=1e-3, alpha=0.2, **kw)
        tr.eng.drop_seed = 4242
        trs.append(tr)
    counts = [_launches(tr, part(0, 5)) for tr in trs]
    assert counts[0] == counts[1] and counts[0]["loss"] >= 2, counts
    for tr in trs:
        tr.step(part(0, 3), stage=3)
    for name in ("master", "opt_m", "opt_v"):
        a, b = getattr(trs[0].eng, name), getattr(trs[1].eng, name)
        assert torch.equal(a, b), (mode, name, int((a != b).sum()))
    for tr in trs:
        assert tr.teng is None and not any(k[0].startswith("kd_") or k[0].startswith("distill_") for k in tr.eng.ws)


# ---- 4
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_the_term_moves_the_student_reproducibly_and_never_the_teacher(mode):
    lr = 1e-3
    runs = []
    for w in (0.5, 0.5, 0.0):
        teacher = build("bf16", shift=0.02) if w else None
        before = None if teacher is None else teacher.engine().master.clone()
        tr = MMTGTrainer(build(mode, 0.1), lr=lr, alpha=0.2, distill_weight=w, distill_teacher=teacher, distill_scale=2.0)
        tr.eng.drop_seed = 4242
        for b in (part(0, 5), part(0, 3)):
            tr.step(b, stage=3)
        runs.append(tr.eng)
        if teacher is not None:
            assert torch.equal(teacher.engine().master, before) and teacher.engine().opt_m is None       # bit-unchanged, no optimizer state
            sd = tr.state_dict()
            assert sd["layout_total"] == tr.eng.layout.total and sd["exp_avg"].numel() == tr.eng.layout.total
    for name in ("master", "opt_m", "opt_v"):
        a, b = getattr(runs[0], name), getattr(runs[1], name)
        assert torch.equal(a, b), (mode, name, int((a != b).sum()))
    assert float((runs[0].master - runs[2].master).abs().max()) > 0.5 * lr


# ---- 5
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_a_window_is_the_big_batch_with_the_term(mode):
    """k = 2 over 32 + 32 rows against one step on the 64 rows, with the bounds of tests/test_accum_gpu.py's
    test_a_window_is_the_big_batch (the same comparison without the term)"""
    lr, w = 1e-3, 0.5
    teacher = build("bf16", shift=0.02)
    big = MMTGTrainer(build(mode), lr=lr, alpha=0.2, distill_weight=w, distill_teacher=teacher, distill_scale=2.0)
    ob = big.step(part(0, 64, 64), stage=3)
    tr = MMTGTrainer(build(mode), lr=lr, alpha=0.2, distill_weight=w, distill_teacher=teacher, distill_scale=2.0, accumulation_steps=2)
    tr.step(part(0, 32, 64), stage=3)
    tr.step(part(32, 64, 64), stage=3)
    g, ref = tr.eng.grad, big.eng.grad
    cos = float(torch.nn.functional.cosine_similarity(g, ref, dim=0))
    rel = float((g - ref).norm() / ref.norm())
    dp = float((tr.eng.master - big.eng.master).abs().max())
    print("cos %.7f rel %.3e max parameter difference %.3e" % (cos, rel, dp))
    assert cos > 0.99999 and rel < 2e-3, (cos, rel)
    assert dp <= 0.2 * lr, dp
    assert float(tr._count.item()) == float(big._count.item()) == 64.0
    # the window's 'kd' is the row-weighted mean of its micro-batches': the big batch's value up to the logits' own rounding
    assert float(tr.window["kd"]) == pytest.approx(float(ob["kd"]), rel=2e-3 if mode == "bf16" else 1e-5)
    noterm = MMTGTrainer(build(mode), lr=lr, alpha=0.2)
    noterm.step(part(0, 64, 64), stage=3)
    assert float((big.eng.grad - noterm.eng.grad).norm() / noterm.eng.grad.norm()) > 0.05       # ... and the term is in the gradient


# ---- 6
def test_the_trainer_refuses_what_the_term_cannot_do():
    student, teacher = build("bf16"), build("bf16")
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
    with pytest.raises(ValueError, match="distill_scale"):
        MMTGTrainer(student, distill_weight=0.5, distill_teacher=teacher, distill_scale=-1.0)


# ---- 7
def test_twenty_steps_bring_the_student_to_the_guided_teacher():
    """bf16, one fixed batch, a teacher guided at scale 2, no dropout: evaluate_batch()['kd'] after twenty steps at the tiny-model
    tests' lr is below its value before; the run is deterministic"""
    batch = part(0, 5)
    teacher = build("bf16", shift=0.02)
    tr = MMTGTrainer(build("bf16"), lr=1e-3, alpha=0.2, distill_weight=1.0, distill_teacher=teacher, distill_scale=2.0)
    before = float(tr.evaluate_batch(batch)["kd"])
    for _ in range(20):
        tr.step(batch, stage=3)
    after = float(tr.evaluate_batch(batch)["kd"])
    print("kd before %.6f, after twenty steps %.6f" % (before, after))
    assert np.isfinite(after) and after < before
