"""MMTGTrainer(experience_drop=...) and the guided validation loss on the real engine: the tiny 2-layer model with tiny_s5's weights
(V = 160, D = 768, P = 15, L = 221), the 5-row synthetic batch tests/test_cl_gpu.py uses, f32 and bf16 modes.  The kernels alone are
in tests/test_cfg_ops_gpu.py, the host side in tests/test_cfg_cpu.py; the restatement, the reference and its bounds in tests/cfg_ref.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_ref as R  # noqa: E402
from helpers import load_case  # noqa: E402
from mmtg_amd import MMTG, hip, synth  # noqa: E402
from mmtg_amd.generate import without_experience  # noqa: E402
from mmtg_amd.trainer import MMTGTrainer  # noqa: E402

DEV = "cuda"
MODES = ["f32", "bf16"]
PROBS = (0.3, 0.2, 0.2)


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


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def zeroed(batch, codes):
    """the batch with the images (bit 0) and texts (bit 1) of the coded rows zeroed, on the host's side of the engine"""
    codes = torch.as_tensor(np.asarray(codes)).to(batch["img_embs"].device)
    out = dict(batch)
    for key, bit in (("img_embs", 1), ("r_embs", 2)):
        t = batch[key].clone()
        t[(codes & bit) != 0] = 0
        out[key] = t
    return out


def no_experience(batch):
    """generate.without_experience of the batch's rows, beside the batch's other keys"""
    neg = without_experience({k: v.cpu().numpy() for k, v in batch.items()})
    return dict(batch, img_embs=neg["img_embs"].to(DEV), r_embs=neg["r_embs"].to(DEV))


@functools.lru_cache(maxsize=None)
def seed_with_all_codes(n=5, probs=PROBS):
    """a drop_seed whose next forward draws the codes 0, 1, 2 and 3 among n rows (found with the restatement, on the CPU)"""
    for s in range(1, 100000):
        if set(R.engine_codes(s, n, probs).tolist()) == {0, 1, 2, 3}:
            return s
    raise AssertionError("no seed")


def _kl_close(x, y, rows, heads, kl=None, alpha=1.0):
    """The kl scalar is the one value of a forward that is not bit-reproducible: mmtg_alpha_attn_fwd adds its n = 2 * rows * heads
    non-negative terms with fp32 atomics, in the order the waves finish (measured on an MI355X: 24 identical forwards of one engine
    give 4 different bit patterns in f32 and 3 in bf16, on the plain batch as on a zeroed one).  Two sums of the same terms are each
    within (n - 1) 2^-24 kl of the exact sum.  x and y are two such kl, or (kl and alpha given) two values loss + alpha * kl with
    equal loss: the product and the sum round once more each."""
    x, y = float(x), float(y)
    n = 2 * rows * heads
    ref = max(abs(x), abs(y)) if kl is None else abs(float(kl))
    return abs(x - y) <= alpha * 2.0 * (n - 1) * R.EPS * ref + 4.0 * R.EPS * max(abs(x), abs(y))


def _same_state(a, b, what=""):
    for name in ("master", "opt_m", "opt_v"):
        x, y = getattr(a.eng, name), getattr(b.eng, name)
        assert torch.equal(x, y), (what, name, int((x != y).sum()))


# ---- 1
@pytest.mark.parametrize("mode", MODES)
def test_the_forward_is_the_zeroed_batch_s_forward(mode):
    batch = part(0, 5)
    src = {k: batch[k].clone() for k in ("img_embs", "r_embs")}
    eng = MMTGTrainer(build(mode, 0.1), lr=0.0, alpha=0.2).eng
    seed = seed_with_all_codes()
    got, kls = [], []
    for drop in (True, False):
        eng.drop_seed = seed
        if drop:
            a = eng.forward(batch, train_flag=True, training=True, logits_f32=False, exp_drop=PROBS)
            codes = a["exp_drop"].cpu().numpy().copy()
            assert a["exp_drop"].dtype == torch.int32 and np.array_equal(codes, R.engine_codes(seed, 5, PROBS))
            assert set(codes.tolist()) == {0, 1, 2, 3}
        else:
            a = eng.forward(zeroed(batch, codes), train_flag=True, training=True, logits_f32=False)
            assert "exp_drop" not in a
        sc = eng.loss(batch["rating"], 3, batch_den=5)
        # (kl's TERMS bit for bit -- the attention probabilities they are summed from -- and the scalar within its atomics' order)
        got.append([_bits(a["logits"]).clone(), _bits(sc).clone(), _bits(a["sample_ce"]).clone(), _bits(a["c"]).clone()]
                   + [_bits(a["alpha"][m][2]).clone() for m in ("img", "text")])
        kls.append(float(a["kl"]))
    for x, y in zip(*got):
        assert torch.equal(x, y)
    assert _kl_close(kls[0], kls[1], 5, eng.sh.heads) and kls[0] > 0
    for k, v in src.items():
        assert torch.equal(batch[k], v)                 # the caller's tensors are never modified
    # exp_drop acts whatever `training` says, and a triple of zeros is no call at all
    eng.forward(batch, train_flag=True, training=False, exp_drop=(1.0, 0.0, 0.0))
    assert bool((eng.act["exp_drop"] == 3).all())
    eng.forward(batch, train_flag=True, training=False, exp_drop=(0.0, 0.0, 0.0))
    assert "exp_drop" not in eng.act


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
    """experience_drop=0.0 against the keyword left out: equal launch counts per step in every category of the library's profiler,
    after two steps with dropout on equal bits in the parameters and both moments, and no buffer of the feature.  With it on only the
    category of the cast and drop launches differs: bf16 replaces the two casts of the channels by one launch, f32 (which passes the
    caller's tensors on) gains one."""
    trs = []
    for kw in ({"experience_drop": 0.0}, {}):
        tr = MMTGTrainer(build(mode, 0.1), lr=1e-3, alpha=0.2, **kw)
        tr.eng.drop_seed = 4242
        trs.append(tr)
    counts = [_launches(tr, part(0, 5)) for tr in trs]
    assert counts[0] == counts[1], counts
    for tr in trs:
        out = tr.step(part(0, 3), stage=3)
        assert sorted(out) == ["kl", "lm_loss", "loss"]
    _same_state(trs[0], trs[1], mode)
    for tr in trs:
        assert not any(k[0].startswith(("exp_drop", "guided")) for k in tr.eng.ws) and "exp_drop" not in tr.eng.act
    on = MMTGTrainer(build(mode, 0.1), lr=1e-3, alpha=0.2, experience_drop=0.1)
    c = _launches(on, part(0, 5))
    assert c["misc"] == counts[0]["misc"] + (1 if mode == "f32" else -1), (c, counts[0])
    assert {k: v for k, v in c.items() if k != "misc"} == {k: v for k, v in counts[0].items() if k != "misc"}, (c, counts[0])
    assert ("exp_drop_code", torch.int32) in on.eng.ws


# ---- 3
@pytest.mark.parametrize("mode", MODES)
def test_dropping_every_row_is_a_step_on_without_experience(mode):
    batch = part(0, 5)
    a = MMTGTrainer(build(mode, 0.1), lr=1e-3, alpha=0.2, experience_drop=1.0)
    b = MMTGTrainer(build(mode, 0.1), lr=1e-3, alpha=0.2)
    a.eng.drop_seed = b.eng.drop_seed = 4242
    oa = a.step(batch, stage=3)
    ob = b.step(no_experience(batch), stage=3)
    assert bool((oa["experience_drop"] == 3).all()) and "experience_drop" not in ob
    for k in ("loss", "lm_loss"):
        assert torch.equal(_bits(oa[k]), _bits(ob[k]))
    assert _kl_close(oa["kl"], ob["kl"], 5, a.eng.sh.heads)
    _same_state(a, b, mode)
    # in eval mode the option is off, like the dropout sites
    a.model.eval()
    assert "experience_drop" not in a.step(batch, stage=3)


# ---- 4
def test_reproducibility_and_a_window_s_two_draws():
    batch = part(0, 5)
    seed = seed_with_all_codes()
    runs, outs = [], []
    for s in (seed, seed, seed + 1):
        tr = MMTGTrainer(build("bf16", 0.1), lr=1e-3, alpha=0.2, experience_drop=PROBS)
        tr.eng.drop_seed = s
        out = tr.step(batch, stage=3)
        assert out["experience_drop"].dtype == torch.int32 and out["experience_drop"].is_cuda and "experience_drop" not in tr.window
        outs.append(out["experience_drop"].cpu().numpy().copy())
        tr.step(part(0, 3), stage=3)
        runs.append(tr)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], R.engine_codes(seed, 5, PROBS))
    _same_state(runs[0], runs[1])
    assert np.array_equal(outs[2], R.engine_codes(seed + 1, 5, PROBS)) and not np.array_equal(outs[0], outs[2])
    # a window of two micro-steps: each forward draws at its own step seed
    tr = MMTGTrainer(build("bf16", 0.1), lr=1e-3, alpha=0.2, experience_drop=PROBS, accumulation_steps=2)
    tr.eng.drop_seed = seed
    c1 = tr.step(batch, stage=3)["experience_drop"].cpu().numpy().copy()
    c2 = tr.step(batch, stage=3)["experience_drop"].cpu().numpy().copy()
    assert np.array_equal(c1, R.engine_codes(seed, 5, PROBS)) and np.array_equal(c2, R.engine_codes(R.next_step_seed(seed), 5, PROBS))
    assert not np.array_equal(c1, c2) and tr.micro_step == 0 and tr.window["rows"] == 10


# ---- 5
def test_resume_continues_bit_exactly():
    """bf16, dropout on: two steps, checkpoint, one more step -- a fresh model and trainer that load the checkpoint and run that step
    hold the same bits in the parameters and both moments, and draw the same codes"""
    A, B = part(0, 3), part(3, 5)
    kw = dict(lr=1e-3, alpha=0.2, warmup_steps=2, total_steps=10, experience_drop=(0.4, 0.2, 0.2))
    model = build("bf16", 0.1)
    tr = MMTGTrainer(model, **kw)
    tr.eng.drop_seed = 4242
    tr.step(A, stage=3)
    tr.step(B, stage=3)
    sd_t = tr.state_dict()
    sd_m = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert sd_t["hparams"]["experience_drop"] == (0.4, 0.2, 0.2)
    c1 = tr.step(A, stage=3)["experience_drop"].cpu()
    model2 = build("bf16", 0.1)
    model2.load_state_dict(sd_m)
    tr2 = MMTGTrainer(model2, **kw)
    tr2.load_state_dict(sd_t)
    c2 = tr2.step(A, stage=3)["experience_drop"].cpu()
    assert torch.equal(c1, c2)
    _same_state(tr, tr2)
    other = MMTGTrainer(build("bf16", 0.1), lr=1e-3, experience_drop=0.25)
    other.load_state_dict(sd_t)
    assert other.experience_drop == (0.25, 0.0, 0.0)                # the trainer's own value stays


# ---- 6
def test_together_with_the_other_options():
    tr = MMTGTrainer(build("bf16", 0.1), lr=1e-3, alpha=0.2, ul_weight=0.5, cl_weight=0.5, accumulation_steps=2, ema_decay=0.99,
                     experience_drop=PROBS)
    for b in (part(0, 3), part(3, 5)):
        out = tr.step(b, stage=3)
        assert sorted(out) == ["cl", "experience_drop", "kl", "lm_loss", "loss", "ul"]
        assert all(bool(torch.isfinite(v).all()) for k, v in out.items() if k != "experience_drop")
        assert out["experience_drop"].shape == (int(b["rating"].shape[0]),)
    assert sorted(tr.window) == ["cl", "kl", "lm_loss", "loss", "rows", "ul"] and tr.ema_updates == 1
    assert bool(torch.isfinite(tr.eng.master).all()) and bool(torch.isfinite(tr.eng.ema).all())


# ---- 7
def test_a_step_in_bf16x3f():
    tr = MMTGTrainer(build("bf16x3f", 0.1), lr=1e-3, alpha=0.2, experience_drop=PROBS)
    tr.eng.drop_seed = seed_with_all_codes()
    batch = part(0, 5)
    src = batch["img_embs"].clone()
    out = tr.step(batch, stage=3)
    assert np.array_equal(out["experience_drop"].cpu().numpy(), R.engine_codes(seed_with_all_codes(), 5, PROBS))
    assert bool(torch.isfinite(tr.eng.grad).all()) and bool(torch.isfinite(tr.eng.master).all()) and float(tr.eng.grad.abs().max()) > 0
    assert torch.equal(batch["img_embs"], src)
    assert ("xi", torch.float32) in tr.eng.ws                       # the f32 modes write named buffers of the engine's own


# ---- 8
@pytest.mark.parametrize("mode", MODES)
def test_evaluation_without_experience(mode):
    batch = part(0, 5)
    tr = MMTGTrainer(build(mode), lr=0.0, alpha=0.2)
    heads = tr.eng.sh.heads
    runs = {}
    for name, call in (("got", lambda: tr.evaluate_batch(batch, without_experience=True)), ("ref", lambda: tr.evaluate_batch(no_experience(batch))),
                       ("plain", lambda: tr.evaluate_batch(batch))):
        out = call()
        runs[name] = {k: v.detach().cpu().clone() for k, v in out.items()}
        runs[name]["logits"] = _bits(tr.eng.act["logits"]).clone()
    got, ref, plain = runs["got"], runs["ref"], runs["plain"]
    assert sorted(got) == ["kl", "logits", "loss", "total"]
    # every value that is reproducible at all bit for bit; kl, and total through it, within the order of kl's atomics (_kl_close)
    assert torch.equal(got["logits"], ref["logits"]) and torch.equal(_bits(got["loss"]), _bits(ref["loss"]))
    assert _kl_close(got["kl"], ref["kl"], 5, heads) and _kl_close(got["total"], ref["total"], 5, heads, kl=got["kl"], alpha=0.2)
    assert not torch.equal(got["logits"], plain["logits"]) and abs(float(got["total"]) - float(plain["total"])) > 1e-3
    a = tr.evaluate([part(0, 3), part(3, 5)], without_experience=True)
    b = tr.evaluate([no_experience(part(0, 3)), no_experience(part(3, 5))])
    c = tr.evaluate([part(0, 3), part(3, 5)])
    assert a == pytest.approx(b, rel=1e-5) and abs(a[0] - c[0]) > 1e-3


# ---- 9
@pytest.mark.parametrize("mode", MODES)
def test_the_guided_validation_loss(mode):
    """evaluate_guided_batch with scales [0, 1, 2]: scale 1 is the conditional cross-entropy and scale 0 the unconditional one, each
    within the derived bounds (cfg_ref.reference on the engine's own two logits matrices for mmtg_guided_loss, cfg_ref.plain_ce_allow
    for the mean of mmtg_loss_fwd's sample_ce); every scale against the float64 reference; the batch as its own negative gives three
    equal values; evaluate_guided is the row-weighted mean"""
    batch = part(0, 5)
    scales = [0.0, 1.0, 2.0]
    tr = MMTGTrainer(build(mode), lr=0.0, alpha=0.2)
    eng, sh = tr.eng, tr.eng.sh
    out = tr.evaluate_guided_batch(batch, scales)
    assert sorted(out) == ["ce", "ce_cond", "ce_uncond", "rows"] and out["rows"] == 5 and out["ce"].shape == (3,) and out["ce"].is_cuda
    ce, ce_cond, ce_uncond = out["ce"].cpu().double(), float(out["ce_cond"]), float(out["ce_uncond"])
    a = eng.act
    P, L, V = sh.P, a["L"], sh.V
    cond, lse_c, tg = a["logits"].cpu(), a["lse_rows"].cpu(), a["targets"].cpu()
    unc = eng.ws[("guided_uncond_logits", a["logits"].dtype)][:cond.numel()].view(cond.shape).cpu()
    lse_u = eng.ws[("guided_uncond_lse", torch.float32)][:lse_c.numel()].cpu()
    assert cond.dtype == (torch.float32 if mode == "f32" else torch.bfloat16) and not torch.equal(_bits(cond), _bits(unc))
    ref = R.reference(cond, unc, lse_c, lse_u, tg, P, V, scales, 5.0)
    for name, got, key, allow in (("nll", a["guided_nll"], "nll", "allow_nll"), ("sample_ce", a["guided_sample_ce"], "sample_ce", "allow_sample"),
                                  ("ce", out["ce"], "ce", "allow_ce")):
        err = (got.cpu().double() - ref[key]).abs()
        assert bool((err <= ref[allow]).all()), (name, float((err / ref[allow].clamp(min=1e-300)).max()))
    b_cond = float(ref["allow_ce"][1]) + R.plain_ce_allow(cond, lse_c, tg, P, V)
    b_unc = float(ref["allow_ce"][0]) + R.plain_ce_allow(unc, lse_u, tg, P, V)
    print(mode, "ce", ce.tolist(), "ce_cond %.7f (|diff| %.2e, bound %.2e) ce_uncond %.7f (|diff| %.2e, bound %.2e)" % (
        ce_cond, abs(float(ce[1]) - ce_cond), b_cond, ce_uncond, abs(float(ce[0]) - ce_uncond), b_unc))
    assert abs(float(ce[1]) - ce_cond) <= b_cond and abs(float(ce[0]) - ce_uncond) <= b_unc
    assert abs(ce_cond - ce_uncond) > 10 * (b_cond + b_unc)         # ... and the two branches differ by far more than that
    # ce_cond is the mean of the engine's sample_ce of a plain evaluate_batch forward, ce_uncond that of the batch without experience
    tr.evaluate_batch(batch)
    assert torch.equal(_bits(eng.act["sample_ce"].mean()), _bits(out["ce_cond"]))
    tr.evaluate_batch(batch, without_experience=True)
    assert torch.equal(_bits(eng.act["sample_ce"].mean()), _bits(out["ce_uncond"]))
    # the default negative is generate.without_experience of the rows; an input the negative does not name is the batch's own
    neg = no_experience(batch)
    o2 = tr.evaluate_guided_batch(batch, scales, negative_batch={k: neg[k] for k in ("img_embs", "r_embs")})
    assert torch.equal(_bits(o2["ce"]), _bits(out["ce"])) and torch.equal(_bits(o2["ce_uncond"]), _bits(out["ce_uncond"]))
    same = tr.evaluate_guided_batch(batch, scales, negative_batch=batch)
    sb = _bits(same["ce"])
    assert bool((sb == sb[0]).all()) and torch.equal(_bits(same["ce_cond"]), _bits(same["ce_uncond"]))
    # over two batches: the row-weighted combination, one host read, the model's mode restored
    parts = [part(0, 3), part(3, 5)]
    per = [tr.evaluate_guided_batch(p, scales) for p in parts]
    per = [{k: (v.cpu().double() if torch.is_tensor(v) else v) for k, v in o.items()} for o in per]
    for was in (True, False):
        tr.model.train(was)
        res = tr.evaluate_guided(parts, scales)
        assert tr.model.training is was
    assert sorted(res) == ["ce", "ce_cond", "ce_uncond", "rows", "scales"] and res["rows"] == 5 and res["scales"] == scales
    for k in range(3):
        assert res["ce"][k] == pytest.approx(float(3 * per[0]["ce"][k] + 2 * per[1]["ce"][k]) / 5, rel=1e-6)
    for key in ("ce_cond", "ce_uncond"):
        assert res[key] == pytest.approx(float(3 * per[0][key] + 2 * per[1][key]) / 5, rel=1e-6)
    assert tr.evaluate_guided_batch(dict(batch, rating=torch.full_like(batch["rating"], 3)), scales, stage=2) is None
