"""MMTGTrainer.evaluate_modality_guided on the real engine: the tiny 2-layer model with tiny_s5's weights (V = 160, D = 768, P = 15,
L = 221) and the 5-row synthetic batch of tests/test_cfg_gpu.py, f32 and bf16 modes.  The kernel alone is in
tests/test_mgloss_ops_gpu.py, the host side in tests/test_mgloss_cpu.py; the reference and its bounds in tests/mgl_ref.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_ref  # noqa: E402
import mgl_ref as R  # noqa: E402
from test_cfg_gpu import DEV, MODES, _bits, build, no_experience, part  # noqa: E402
from mmtg_amd.generate import without_images, without_texts  # noqa: E402
from mmtg_amd.trainer import MMTGTrainer, best_scale  # noqa: E402

SCALES = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 0.5), (1.5, 3, 0.5)]
FLOATS = [tuple(float(s) for s in t) for t in SCALES]


def _negative(batch, fn):
    """generate.without_images / without_texts of the batch's rows, beside the batch's other keys"""
    neg = fn({k: v.cpu().numpy() for k, v in batch.items()})
    return dict(batch, img_embs=neg["img_embs"].to(DEV), r_embs=neg["r_embs"].to(DEV))


def _named(eng, name, like):
    return eng.ws[(name, like.dtype)][:like.numel()].view(like.shape).cpu()


def _guided_buffers(eng):
    return sorted(k[0] for k in eng.ws if k[0].startswith("guided_neg"))


@pytest.mark.parametrize("mode", MODES)
def test_the_modality_guided_validation_loss(mode):
    batch = part(0, 5)
    tr = MMTGTrainer(build(mode), lr=0.0, alpha=0.2)
    eng, sh = tr.eng, tr.eng.sh
    before = tr.evaluate_guided([part(0, 3), part(3, 5)], [0.0, 1.0, 2.0])
    old = tr.evaluate_guided_batch(batch, [2.0])["ce"].cpu().double()
    out = tr.evaluate_modality_guided_batch(batch, SCALES)
    assert sorted(out) == ["ce", "ce_cond", "ce_negatives", "rows"] and out["rows"] == 5 and out["ce"].shape == (5,) and out["ce"].is_cuda
    assert list(out["ce_negatives"]) == ["u", "i", "t"] and all(v.is_cuda and v.dim() == 0 for v in out["ce_negatives"].values())
    ce, ce_cond = out["ce"].cpu().double(), float(out["ce_cond"])
    a = eng.act
    P, L, V = sh.P, a["L"], sh.V
    cond, lse_c, tg = a["logits"].cpu(), a["lse_rows"].cpu(), a["targets"].cpu()
    assert cond.dtype == (torch.float32 if mode == "f32" else torch.bfloat16)
    negs = [_named(eng, "guided_neg%d_logits" % k, a["logits"]) for k in (1, 2, 3)]
    nlse = [_named(eng, "guided_neg%d_lse" % k, a["lse_rows"]) for k in (1, 2, 3)]
    mats = [cond] + negs
    assert all(not torch.equal(_bits(mats[i]), _bits(mats[j])) for i in range(4) for j in range(i))
    ref = R.reference(mats, [lse_c] + nlse, tg, P, V, FLOATS, 5.0)
    for name, got, key, allow in (("nll", a["guided_nll"], "nll", "allow_nll"), ("sample_ce", a["guided_sample_ce"], "sample_ce", "allow_sample"),
                                  ("ce", out["ce"], "ce", "allow_ce")):
        err = (got.cpu().double() - ref[key]).abs()
        print(mode, name, "worst err / allowed %.3f" % float((err / ref[allow].clamp(min=1e-300)).max()))
        assert tuple(got.shape) == tuple(ref[key].shape) and bool((err <= ref[allow]).all()), name
    # (1, 1, 1) is the conditional cross-entropy; (2, 1, 1) is evaluate_guided_batch at scale 2
    b_cond = float(ref["allow_ce"][0]) + cfg_ref.plain_ce_allow(cond, lse_c, tg, P, V)
    two = cfg_ref.reference(cond, negs[0], lse_c, nlse[0], tg, P, V, [2.0], 5.0)
    b_two = float(ref["allow_ce"][1]) + float(two["allow_ce"][0]) + 1e-12
    print(mode, "ce", ce.tolist(), "ce_cond %.7f (|diff| %.2e, bound %.2e); evaluate_guided_batch at 2: %.7f (|diff| %.2e, bound %.2e)" % (
        ce_cond, abs(float(ce[0]) - ce_cond), b_cond, float(old[0]), abs(float(ce[1]) - float(old[0])), b_two))
    assert abs(float(ce[0]) - ce_cond) <= b_cond and abs(float(ce[1]) - float(old[0])) <= b_two
    assert best_scale({"scales": FLOATS, "ce": ce.tolist(), "rows": 5}) == FLOATS[int(ce.argmin())]
    # each negative's own cross-entropy: the forward on the host-zeroed batch of the decoders' negative prompts
    for name, neg in (("u", no_experience(batch)), ("i", _negative(batch, without_images)), ("t", _negative(batch, without_texts))):
        tr.evaluate_batch(neg)
        assert torch.equal(_bits(eng.act["sample_ce"].mean()), _bits(out["ce_negatives"][name])), name
    tr.evaluate_batch(batch)
    assert torch.equal(_bits(eng.act["sample_ce"].mean()), _bits(out["ce_cond"]))
    # over two unequal batches: the row-weighted combination, the model's mode restored
    parts = [part(0, 3), part(3, 5)]
    per = [tr.evaluate_modality_guided_batch(p, SCALES) for p in parts]
    for was in (True, False):
        tr.model.train(was)
        res = tr.evaluate_modality_guided(parts, SCALES)
        assert tr.model.training is was
    assert sorted(res) == ["ce", "ce_cond", "ce_negatives", "rows", "scales"] and res["rows"] == 5 and res["scales"] == FLOATS
    mean = lambda x, y: float(3 * x.cpu().double() + 2 * y.cpu().double()) / 5
    for g in range(5):
        assert res["ce"][g] == pytest.approx(mean(per[0]["ce"][g], per[1]["ce"][g]), rel=1e-6)
    assert res["ce_cond"] == pytest.approx(mean(per[0]["ce_cond"], per[1]["ce_cond"]), rel=1e-6)
    assert list(res["ce_negatives"]) == ["u", "i", "t"]
    for k in "uit":
        assert res["ce_negatives"][k] == pytest.approx(mean(per[0]["ce_negatives"][k], per[1]["ce_negatives"][k]), rel=1e-6)
    assert best_scale(res) == FLOATS[min(range(5), key=res["ce"].__getitem__)]
    # stage 1 with no surviving row
    flat = dict(batch, rating=torch.full_like(batch["rating"], 3))
    assert tr.evaluate_modality_guided_batch(flat, SCALES, stage=1) is None
    none = tr.evaluate_modality_guided([flat], SCALES, stage=1)
    assert none == {"scales": FLOATS, "ce": [0.0] * 5, "ce_cond": 0.0, "ce_negatives": {"u": 0.0, "i": 0.0, "t": 0.0}, "rows": 0}
    with pytest.raises(ValueError, match="rows == 0"):
        best_scale(none)
    # evaluate_guided is what it was before
    after = tr.evaluate_guided([part(0, 3), part(3, 5)], [0.0, 1.0, 2.0])
    assert after == before


def test_only_the_needed_negatives_run():
    batch = part(0, 5)
    tr = MMTGTrainer(build("bf16"), lr=0.0, alpha=0.2)
    eng = tr.eng
    ones = tr.evaluate_modality_guided_batch(batch, [(1, 1, 1), (1.0, 1.0, 1.0)])
    assert _guided_buffers(eng) == [] and "guided_nll" not in eng.act and ones["ce_negatives"] == {}
    assert ones["ce"].shape == (2,) and bool((_bits(ones["ce"]) == _bits(ones["ce_cond"])).all())
    it = tr.evaluate_modality_guided_batch(batch, [(1, 2, 1), (1, 1, 0.5), (1, 3, 1)])
    assert _guided_buffers(eng) == ["guided_neg1_logits", "guided_neg1_lse", "guided_neg2_logits", "guided_neg2_lse"]
    assert list(it["ce_negatives"]) == ["i", "t"] and eng.act["guided_nll"].shape[0] == 3
    # the image branch alone is the two-matrix launch on the same negative: the bits of the (i, t) launch's tuples with t at 1
    i_only = tr.evaluate_modality_guided_batch(batch, [(1, 2, 1), (1, 1, 1), (1, 3, 1)])
    assert list(i_only["ce_negatives"]) == ["i"] and len(_guided_buffers(eng)) == 4 and eng.act["guided_nll"].shape[0] == 3
    assert torch.equal(_bits(i_only["ce"][[0, 2]]), _bits(it["ce"][[0, 2]]))
    assert torch.equal(_bits(i_only["ce_negatives"]["i"]), _bits(it["ce_negatives"]["i"]))
    # and the experience branch alone is evaluate_guided_batch's distribution, negative and all
    u = tr.evaluate_modality_guided_batch(batch, [(0.0, 1, 1), (2.0, 1, 1)])
    g = tr.evaluate_guided_batch(batch, [0.0, 2.0])
    assert torch.equal(_bits(u["ce_negatives"]["u"]), _bits(g["ce_uncond"])) and torch.equal(_bits(u["ce_cond"]), _bits(g["ce_cond"]))
    res = tr.evaluate_modality_guided([part(0, 3), part(3, 5)], [(1, 2, 1), (1, 1, 1)])
    assert list(res["ce_negatives"]) == ["i"] and res["rows"] == 5 and res["ce"][1] == pytest.approx(res["ce_cond"], rel=1e-6)


def test_the_averaged_weights_are_what_averaged_reads():
    parts = [part(0, 3), part(3, 5)]
    tr = MMTGTrainer(build("bf16"), lr=1e-2, alpha=0.2, ema_decay=0.5)
    tr.step(part(0, 5), stage=3)
    tr.step(part(0, 5), stage=3)
    was = tr.model.training
    last = tr.evaluate_modality_guided(parts, SCALES)
    avg = tr.evaluate_modality_guided(parts, SCALES, averaged=True)
    with tr.averaged_weights():
        inside = tr.evaluate_modality_guided(parts, SCALES)
    assert avg == inside and avg != last and avg["rows"] == 5 and tr.model.training is was
    assert tr.evaluate_modality_guided(parts, SCALES) == last            # the last iterate is back
