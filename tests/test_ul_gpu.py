"""MMTGTrainer(ul_weight=...) on the real engine: the tiny 2-layer model with tiny_s5's weights (V = 160, P = 15, L = 221), 5-row
synthetic batches whose lyrics repeat ids by themselves, f32 and bf16 modes.  The kernels alone are in tests/test_ul_ops_gpu.py, the
host side in tests/test_ul_cpu.py; the reference and its bounds in tests/ul_ref.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ul_ref as R  # noqa: E402
from helpers import load_case  # noqa: E402
from mmtg_amd import MMTG, hip, synth  # noqa: E402
from mmtg_amd.trainer import MMTGTrainer  # noqa: E402

DEV = "cuda"
MODES = ["f32", "bf16"]


@functools.lru_cache(maxsize=None)
def _case():
    fx, meta, mcfg, gcfg, dcfg, weights, table, _ = load_case("tiny_s5")
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    return meta, mcfg, gcfg, dcfg, sd, table


def build(mode, pdrop=0.0):
    meta, mcfg, gcfg, dcfg, sd, table = _case()
    gcfg = dict(gcfg, embd_pdrop=pdrop, attn_pdrop=pdrop, resid_pdrop=pdrop)
    model = MMTG(mcfg, dcfg, meta["V"], train_flag=True, gpt2_config=gcfg, token_table=table, compute_dtype=mode)
    model.load_state_dict(sd)
    model.to(DEV)
    model.train(pdrop > 0)
    return model


@functools.lru_cache(maxsize=None)
def rows5(seed=7):
    meta, mcfg, gcfg, dcfg, sd, table = _case()
    nb = synth.make_batch(5, mcfg, dcfg, meta["V"], seed=seed)
    return {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nb.items()}


def part(lo, hi):
    return {k: v[lo:hi] for k, v in rows5().items()}


def _within(name, got, ref, allow):
    err = (got.double() - ref).abs()
    assert bool((err <= allow).all()), "%s: %d outside the bound, worst err/allowed %.3g" % (
        name, int((err > allow).sum()), float((err / allow.clamp(min=1e-300)).max()))


# ---- 1
@pytest.mark.parametrize("mode", MODES)
def test_the_engine_follows_the_rule_on_its_own_logits(mode):
    """ul, the row sums and d(logits) of the engine against ul_ref on the logits and the lse the engine itself produced (bf16: the
    logits are read back before the backward overwrites them); step() returns the same 'ul' bits"""
    w, n = 0.5, 5
    batch = part(0, n)
    tr = MMTGTrainer(build(mode), lr=0.0, alpha=0.2, ul_weight=w)
    eng, sh = tr.eng, tr.eng.sh
    eng.forward(batch, train_flag=True, training=False, logits_f32=False)
    eng.loss(batch["rating"], 3, batch_den=n)
    ul = eng.ul_loss(batch_den=n)
    a = eng.act
    V, P, L, Vp = sh.V, sh.P, a["L"], eng.layout.Vpad
    x = a["logits"].detach().cpu().clone()
    assert x.dtype == (torch.float32 if mode == "f32" else torch.bfloat16) and x.shape == (n * (P + L), Vp)
    lse, tg, topic, coef = a["lse_rows"].cpu(), a["targets"].cpu(), a["topic_ids"].cpu(), a["coef"].cpu()
    fw = R.forward(x, lse, tg, P, V, R.DEFAULT_EXCLUDE, float(n))
    assert int(fw["n"].max()) > 50 and float(fw["ul"]) > 0.1               # the lyrics do repeat
    print(mode, "ul %.6f ref %.6f, candidates per row up to %d" % (float(ul), float(fw["ul"]), int(fw["n"].max())))
    _within("ul_row", a["ul_row"].cpu(), fw["ul_row"], fw["allow_row"])
    _within("S", a["ul_S"].cpu(), fw["S"], fw["allow_S"])
    _within("ul_sample", a["ul_sample"].cpu(), fw["ul_sample"], fw["allow_sample"])
    _within("ul", ul.cpu(), fw["ul"].reshape(1), fw["allow_ul"].reshape(1))
    ul_bits = ul.cpu().clone()
    S32 = a["ul_S"].cpu().clone()
    u = w / ((L - 1) * n) * float(n)
    dl = eng.loss_backward_ul(float(n), 0.0, u)
    assert (dl.data_ptr() == a["logits"].data_ptr()) == (mode == "bf16")    # f32: the logits survive; bf16: rewritten in place
    d, allow, rc = R.backward(fw, S32, topic, tg, coef, float(n), 0.0, u, P, V)
    got = dl.cpu()
    _within("d(logits)", got[:, :V], d, R.out_allow(d, allow, "f32" if mode == "f32" else "bf16"))
    assert bool((got[:, V:] == 0).all())
    plain = MMTGTrainer(build(mode), lr=0.0, alpha=0.2)
    plain.eng.forward(batch, train_flag=True, training=False, logits_f32=False)
    plain.eng.loss(batch["rating"], 3, batch_den=n)
    base = plain.eng.loss_backward(float(n)).cpu()
    moved = (got[:, :V].double() - base[:, :V].double()).abs().sum()
    assert float(moved) > 0.1 * float(base[:, :V].double().abs().sum()), "the term hardly changed d(logits)"
    out = tr.step(batch, stage=3)
    assert torch.equal(out["ul"].cpu().reshape(1).view(torch.int32), ul_bits.view(torch.int32))
    assert sorted(out) == ["kl", "lm_loss", "loss", "ul"] and float(tr.window["ul"]) == float(out["ul"])
    ev = tr.evaluate_batch(batch)
    assert float(ev["ul"]) == float(ul_bits) and float(ev["total"]) == pytest.approx(float(ev["loss"]) + 0.2 * float(ev["kl"]), rel=1e-6)


# ---- 2
def _launches(tr, batch):
    hip.prof_enable(True)
    try:
        tr.step(batch, stage=3)
        rec = hip.prof_read()
    finally:
        hip.prof_enable(False)
    return {k: v["launches"] for k, v in rec.items()}


@pytest.mark.parametrize("mode", MODES)
def test_the_default_is_today_s_trainer(mode):
    """ul_weight=0.0 against the keyword left out: equal launch counts per step in every category of the library's profiler, and after
    two steps with dropout on equal bits in the parameters and both moments; no buffer of the term exists"""
    trs = []
    for kw in ({"ul_weight": 0.0}, {}):
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
        assert tr.eng.ul_exclude is None and not any(k[0].startswith("ul_") for k in tr.eng.ws)
    # the term costs one launch more in the loss category (its forward; the backward replaces today's)
    on = MMTGTrainer(build(mode, 0.1), lr=1e-3, alpha=0.2, ul_weight=0.5)
    c = _launches(on, part(0, 5))
    assert c["loss"] == counts[0]["loss"] + 1 and {k: v for k, v in c.items() if k != "loss"} == {k: v for k, v in counts[0].items() if k != "loss"}, (c, counts[0])


# ---- 3
@pytest.mark.parametrize("mode", MODES)
def test_the_term_moves_the_parameters_reproducibly(mode):
    lr = 1e-3
    runs = []
    for w in (0.5, 0.5, 0.0):
        tr = MMTGTrainer(build(mode, 0.1), lr=lr, alpha=0.2, ul_weight=w)
        tr.eng.drop_seed = 4242
        for b in (part(0, 5), part(0, 3)):
            tr.step(b, stage=3)
        runs.append(tr.eng)
    for name in ("master", "opt_m", "opt_v"):
        a, b = getattr(runs[0], name), getattr(runs[1], name)
        assert torch.equal(a, b), (mode, name, int((a != b).sum()))
    assert float((runs[0].master - runs[2].master).abs().max()) > 0.5 * lr


# ---- 4
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_a_window_is_the_big_batch_with_the_term(mode):
    """k = 2 over 3 + 2 rows against one step on the five rows, with the bounds of tests/test_accum_gpu.py's
    test_a_window_is_the_big_batch (the same comparison without the term)"""
    lr, w = 1e-3, 0.5
    big = MMTGTrainer(build(mode), lr=lr, alpha=0.2, ul_weight=w)
    ob = big.step(part(0, 5), stage=3)
    tr = MMTGTrainer(build(mode), lr=lr, alpha=0.2, ul_weight=w, accumulation_steps=2)
    tr.step(part(0, 3), stage=3)
    tr.step(part(3, 5), stage=3)
    g, ref = tr.eng.grad, big.eng.grad
    cos = float(torch.nn.functional.cosine_similarity(g, ref, dim=0))
    rel = float((g - ref).norm() / ref.norm())
    dp = float((tr.eng.master - big.eng.master).abs().max())
    print("cos %.7f rel %.3e max parameter difference %.3e" % (cos, rel, dp))
    assert cos > 0.99999 and rel < 2e-3, (cos, rel)
    assert dp <= 0.2 * lr, dp
    assert float(tr._count.item()) == float(big._count.item()) == 5.0
    # the window's 'ul' is the row-weighted mean of its micro-batches': the big batch's value up to the logits' own rounding
    assert float(tr.window["ul"]) == pytest.approx(float(ob["ul"]), rel=2e-3 if mode == "bf16" else 1e-5)
    noterm = MMTGTrainer(build(mode), lr=lr, alpha=0.2)
    noterm.step(part(0, 5), stage=3)
    assert float((big.eng.grad - noterm.eng.grad).norm() / noterm.eng.grad.norm()) > 0.05       # ... and the term is in the gradient


# ---- 5
def test_resume_continues_bit_exactly():
    """bf16, dropout on: two steps, checkpoint, one more step -- a fresh model and trainer that load the checkpoint and run that step
    hold the same bits in the parameters and both moments"""
    A, B = part(0, 3), part(3, 5)
    kw = dict(lr=1e-3, alpha=0.2, warmup_steps=2, total_steps=10, ul_weight=0.5, ul_exclude_ids=(0, 1, 2))
    model = build("bf16", 0.1)
    tr = MMTGTrainer(model, **kw)
    tr.eng.drop_seed = 4242
    tr.step(A, stage=3)
    tr.step(B, stage=3)
    sd_t = tr.state_dict()
    sd_m = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert sd_t["hparams"]["ul_weight"] == 0.5 and sd_t["hparams"]["ul_exclude_ids"] == (0, 1, 2)
    tr.step(A, stage=3)
    model2 = build("bf16", 0.1)
    model2.load_state_dict(sd_m)
    tr2 = MMTGTrainer(model2, **kw)
    tr2.load_state_dict(sd_t)
    o2 = tr2.step(A, stage=3)
    for name in ("master", "opt_m", "opt_v"):
        a, b = getattr(tr.eng, name), getattr(tr2.eng, name)
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert torch.isfinite(o2["ul"]) and float(o2["ul"]) > 0
