"""The weight average through the trainer (MMTGTrainer(ema_decay=...)) on the GPU: it does not disturb training, follows its
recurrence within the bound of tests/ema_ref.py, tracks frozen tensors and pads bit for bit, counts windows, and -- swapped into
the masters by averaged_weights() -- is what evaluation and generation read, with every derived copy re-derived.

The tiny 2-layer model with tiny_s5's weights and configuration, 5-row synthetic batches, lr 1e-3 (as tests/test_accum_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ema_ref import check_update  # noqa: E402
from helpers import batch_to_torch, load_case  # noqa: E402
from mmtg_amd import MMTG, synth  # noqa: E402
from mmtg_amd.decode import GreedyDecoder  # noqa: E402
from mmtg_amd.trainer import MMTGTrainer, load_checkpoint, save_checkpoint  # noqa: E402

DEV = "cuda"
MODES = ["bf16", "bf16x3f", "bf16x3", "f32"]
LR = 1e-3


@functools.lru_cache(maxsize=None)
def _case():
    fx, meta, mcfg, gcfg, dcfg, weights, table, batch = load_case("tiny_s5")
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    return meta, mcfg, gcfg, dcfg, sd, table, batch


def build(mode, pdrop=0.0, state=None):
    """tiny_s5's model (or the same model with `state` loaded); pdrop > 0 = GPT-2's three dropouts on, in training mode"""
    meta, mcfg, gcfg, dcfg, sd, table, _ = _case()
    gcfg = dict(gcfg, embd_pdrop=pdrop, attn_pdrop=pdrop, resid_pdrop=pdrop)
    model = MMTG(mcfg, dcfg, meta["V"], train_flag=True, gpt2_config=gcfg, token_table=table, compute_dtype=mode)
    model.load_state_dict(sd if state is None else state)
    model.to(DEV)
    model.train(pdrop > 0)
    return model


@functools.lru_cache(maxsize=None)
def rows5(seed=7):
    meta, mcfg, gcfg, dcfg, sd, table, _ = _case()
    nb = synth.make_batch(5, mcfg, dcfg, meta["V"], seed=seed)
    return {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nb.items()}


def bits(t):
    return t.detach().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def trained(mode, steps=3, **kw):
    """a trainer with an average after `steps` steps on batches of seeds 7, 8, ..."""
    tr = MMTGTrainer(build(mode), lr=LR, alpha=0.2, ema_decay=0.9, **kw)
    for s in range(steps):
        tr.step(rows5(7 + s), stage=3)
    return tr


def kl_rel(eng, rows):
    """The KL scalar is the one output here that is not reproducible bit for bit: every workgroup of the two alpha-attention
    launches adds its non-negative share with an fp32 atomic, so the value depends on the order of arrival.  A sum of N
    non-negative terms is within (N - 1) 2^-24 of the exact sum in any order; two orders differ by at most twice that, relative."""
    n = 2 * rows * eng.sh.heads
    return 2.0 * n * 2.0 ** -24


def close_kl(a, b, eng, rows):
    a, b = float(a), float(b)
    return abs(a - b) <= kl_rel(eng, rows) * max(abs(a), abs(b))


def decay_at(t, decay=0.9, warmup=True):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


# ---- 1
@pytest.mark.parametrize("mode", MODES)
def test_the_average_does_not_disturb_training(mode):
    trs = []
    for kw in ({"ema_decay": 0.9}, {}):
        tr = MMTGTrainer(build(mode, 0.1), lr=LR, alpha=0.2, **kw)
        tr.eng.drop_seed = 4242
        trs.append(tr)
    for step in range(3):
        outs = [tr.step(rows5(7 + step), stage=3) for tr in trs]
        assert same_bits(trs[0].eng.master, trs[1].eng.master), (mode, step)
        assert same_bits(outs[0]["loss"], outs[1]["loss"]) and same_bits(outs[0]["lm_loss"], outs[1]["lm_loss"])
        assert close_kl(outs[0]["kl"], outs[1]["kl"], trs[0].eng, 5)
    assert trs[0].ema_updates == 3 and trs[0].eng.ema is not None and trs[1].eng.ema is None and trs[1].ema_updates == 0
    assert not same_bits(trs[0].eng.ema, trs[0].eng.master)


# ---- 2
@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "constant"])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_the_recurrence(mode, warmup):
    tr = MMTGTrainer(build(mode), lr=LR, alpha=0.2, ema_decay=0.9, ema_warmup=warmup)
    eng = tr.eng
    assert eng.ema is None
    prev = eng.master.cpu().numpy().copy()               # the average starts as the initial weights
    for s in range(4):
        tr.step(rows5(7 + s), stage=3)
        master, got = eng.master.cpu().numpy(), eng.ema.cpu().numpy()
        assert (master != prev).any()
        check_update(prev, master, 1.0 - decay_at(s, 0.9, warmup), got, "%s, step %d" % (mode, s + 1))
        prev = got.copy()
    assert tr.ema_updates == 4


# ---- 3
def test_frozen_tensors_and_pads_track_the_master():
    tr = MMTGTrainer(build("bf16"), lr=LR, alpha=0.2, ema_decay=0.9, param_groups=[{"params": "decoder.gpt2.*", "frozen": True}])
    eng, lay = tr.eng, tr.eng.layout
    init = eng.master.clone()
    for s in range(3):
        tr.step(rows5(7 + s), stage=3)
    trainable = torch.zeros(lay.total, dtype=torch.bool, device=DEV)
    moved = 0
    for key, (off, _, n) in lay.entries.items():
        e, m = lay.view(eng.ema, key), lay.view(eng.master, key)
        if key.startswith("decoder.gpt2."):
            assert same_bits(e, m) and same_bits(m, lay.view(init, key)), key
        else:
            trainable[off:off + n] = True
            # The one-element att_matrices.*.bias keys shift the three scores of one softmax alike: their gradient is zero but for
            # rounding (tests/test_param_groups_gpu.py::test_trainer_frozen_decoder), they move by an ulp or not at all, and an
            # average one ulp behind is rounded onto the master by the next update (w >= 0.75 here).  Every other tensor that
            # moved has elements that moved by far more than that, and its average lags behind.
            if key.startswith("mm_atten_layer.att_matrices.") and key.endswith(".bias"):
                continue
            assert not same_bits(m, lay.view(init, key)), key
            moved += 1
            assert not same_bits(e, m), key
    print("%d trainable tensors moved, and their averages lag behind" % moved)
    assert moved > 0
    # everything outside the trainable tensors -- frozen tensors, the gaps between packs, wte's tail pad -- keeps the master's bits
    assert int((~trainable).sum()) > sum(e[2] for k, e in lay.entries.items() if k.startswith("decoder.gpt2."))      # there are pads
    assert torch.equal(bits(eng.ema)[~trainable], bits(eng.master)[~trainable])


# ---- 4
def test_the_average_counts_windows():
    trs = [MMTGTrainer(build("bf16"), lr=LR, alpha=0.2, ema_decay=0.9, accumulation_steps=2) for _ in range(2)]
    a = trs[0]
    init = a.eng.master.cpu().numpy().copy()
    halves = [{k: v[lo:hi] for k, v in rows5(seed).items()} for seed in (7, 8) for lo, hi in ((0, 3), (3, 5))]
    closed = []
    for i, b in enumerate(halves):
        for tr in trs:
            tr.step(b, stage=3)
        if i % 2 == 0:
            assert a.ema_updates == i // 2 and (a.eng.ema is None) == (i == 0)      # a micro-step moves nothing
        else:
            closed.append((a.eng.master.cpu().numpy().copy(), a.eng.ema.cpu().numpy().copy()))
    assert a.ema_updates == 2 and a.eng.step_count == 2
    assert same_bits(trs[0].eng.ema, trs[1].eng.ema) and same_bits(trs[0].eng.master, trs[1].eng.master)
    check_update(init, closed[0][0], 1.0 - decay_at(0), closed[0][1], "window 1")
    check_update(closed[0][1], closed[1][0], 1.0 - decay_at(1), closed[1][1], "window 2")


# ---- 5
def eval_outputs(tr, batch):
    """the eval-mode outputs that read the weights: evaluate_batch's loss and the model's forward (LM loss, logits) -- compared
    bit for bit -- and the two KL scalars, compared within kl_rel"""
    out = tr.evaluate_batch(batch, stage=3)
    loss, kl0 = out["loss"].clone(), float(out["kl"])          # (views of the engine's scalars: the next forward overwrites them)
    with torch.no_grad():
        lm, kl, logits = tr.model(batch)
    return [loss, lm.clone(), logits.clone()], [kl0, float(kl)]


def same_outputs(a, b, eng):
    return all(same_bits(x, y) for x, y in zip(a[0], b[0])) and all(close_kl(x, y, eng, 5) for x, y in zip(a[1], b[1]))


def same_evaluation(a, b, eng):
    """evaluate()'s (total, alpha * kl) means: the KL part within kl_rel, the total within that and the four roundings on its way"""
    slack = kl_rel(eng, 5) * max(abs(a[1]), abs(b[1]))
    return abs(a[1] - b[1]) <= slack + 2.0 ** -22 * abs(a[1]) and abs(a[0] - b[0]) <= slack + 2.0 ** -22 * abs(a[0])


@pytest.mark.parametrize("mode", MODES)
def test_the_swap_re_derives_every_copy(mode):
    tr = trained(mode)
    eng = tr.eng
    fixed = rows5(21)
    master = eng.master.clone()
    before = eval_outputs(tr, fixed)
    second = MMTGTrainer(build(mode, state=tr.ema_state_dict()), lr=LR, alpha=0.2)
    want = eval_outputs(second, fixed)
    with tr.averaged_weights():
        assert same_bits(eng.master, second.eng.master) and same_bits(eng.ema, master)
        inside = eval_outputs(tr, fixed)
        ev_inside = tr.evaluate([fixed, rows5(22)], stage=3)
    assert same_outputs(inside, want, eng), mode
    assert all(not same_bits(a, b) for a, b in zip(inside[0], before[0]))          # loss, LM loss and logits: the weights differ
    assert same_bits(eng.master, master)
    after = eval_outputs(tr, fixed)
    assert same_outputs(after, before, eng), mode
    ev_avg, ev_last = tr.evaluate([fixed, rows5(22)], stage=3, averaged=True), tr.evaluate([fixed, rows5(22)], stage=3)
    print("%s: evaluate inside %r, averaged=True %r, last iterate %r" % (mode, ev_inside, ev_avg, ev_last))
    assert same_evaluation(ev_avg, ev_inside, eng)
    assert not same_evaluation(ev_last, ev_inside, eng) and same_bits(eng.master, master)
    tr.step(rows5(7), stage=3)                        # ... and training goes on
    assert tr.ema_updates == 4


# ---- 6
def test_generation_reads_the_averaged_weights():
    from mmtg_amd.generate import generate_samples
    tr = trained("bf16")
    _, _, _, _, _, _, batch = _case()
    tb = {k: v for k, v in batch_to_torch(batch, DEV).items() if k not in ("rating", "targets")}
    rows = [{k: np.asarray(v[r]) for k, v in batch.items() if k not in ("rating", "targets")} for r in range(2)]

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return ["t%d" % int(i) for i in ids]

    greedy = dict(n_samples=1, length=24, temperature=1.0, top_k=1, top_p=0.0, repetition_penalty=1.0, return_scores=True)
    length = 24
    dec = GreedyDecoder(tr.model, max_batch=3, max_len=length)
    last_ids, last_lp = (t.clone() for t in dec.generate(tb, length, return_logprobs=True))
    last_text = generate_samples(tr.model, rows, Tok(), **greedy)
    second = build("bf16", state=tr.ema_state_dict())
    want_ids, want_lp = (t.clone() for t in GreedyDecoder(second, max_batch=3, max_len=length).generate(tb, length, return_logprobs=True))
    want_text = generate_samples(second, rows, Tok(), **greedy)
    with tr.averaged_weights():
        ids, lp = (t.clone() for t in dec.generate(tb, length, return_logprobs=True))
        text = generate_samples(tr.model, rows, Tok(), **greedy)
    assert torch.equal(ids, want_ids) and same_bits(lp, want_lp) and text == want_text
    assert not same_bits(lp, last_lp)                  # the decoder really read other weights
    print("ids differ between the average and the last iterate in %d of %d places" % (int((ids != last_ids).sum()), ids.numel()))
    ids, lp = dec.generate(tb, length, return_logprobs=True)          # the same decoder object, after the context
    assert torch.equal(ids, last_ids) and same_bits(lp, last_lp)
    assert generate_samples(tr.model, rows, Tok(), **greedy) == last_text


# ---- 7
def test_resume_continues_the_average(tmp_path):
    def make():
        tr = MMTGTrainer(build("bf16", 0.1), lr=LR, alpha=0.2, ema_decay=0.9)
        return tr

    a = make()
    a.eng.drop_seed = 99
    for s in range(2):
        a.step(rows5(7 + s), stage=3)
    path = str(tmp_path / "ckpt.pt")
    save_checkpoint(path, a.model, a)
    for s in range(2, 4):
        a.step(rows5(7 + s), stage=3)
    b = make()
    ckpt = load_checkpoint(path, b.model, b)
    assert ckpt["trainer"]["ema"]["updates"] == 2 and ckpt["trainer"]["ema"]["average"].shape == (b.eng.layout.total,)
    assert b.ema_updates == 2 and b.eng.ema is not None
    for s in range(2, 4):
        b.step(rows5(7 + s), stage=3)
    assert same_bits(a.eng.master, b.eng.master) and same_bits(a.eng.ema, b.eng.ema) and a.ema_updates == b.ema_updates == 4
    # the averaged model as a checkpoint, in both key styles; 'trainer' still holds the raw state
    avg = a.ema_state_dict()
    for ref_compat in (False, True):
        p = str(tmp_path / ("avg%d.pt" % ref_compat))
        save_checkpoint(p, a.model, a, reference_compatible=ref_compat, averaged=True)
        raw = torch.load(p, map_location="cpu", weights_only=False)
        assert same_bits(raw["trainer"]["ema"]["average"], a.eng.ema.cpu()) and same_bits(raw["trainer"]["exp_avg"], a.eng.opt_m.cpu())
        if ref_compat:
            assert all(k.startswith("module.") for k in raw["model"])
            assert all(same_bits(raw["model"]["module." + k], v) for k, v in avg.items())
            assert "module.decoder.gpt2.transformer.h.0.attn.masked_bias" in raw["model"]
        else:
            assert list(raw["model"]) == list(avg)
        plain = build("bf16")
        load_checkpoint(p, plain)
        got = plain.state_dict()
        assert list(got) == list(avg) and all(same_bits(got[k].cpu(), avg[k]) for k in avg)
        assert same_bits(plain.engine().master, a.eng.ema)          # pads included: they are zero in both
    assert not same_bits(a.eng.master, a.eng.ema)
    with pytest.raises(RuntimeError, match="ema_decay=None"):
        save_checkpoint(str(tmp_path / "none.pt"), a.model, MMTGTrainer(plain, lr=LR), averaged=True)
