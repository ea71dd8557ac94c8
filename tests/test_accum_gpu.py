"""Gradient accumulation in the fused trainer (MMTGTrainer(accumulation_steps=k)) on the GPU: a window of k micro-steps zeroes once,
adds the micro-batches' row sums through the engine's accumulating backward, and steps once over the window's row count.

The tiny 2-layer model with tiny_s5's weights and configuration; 5-row synthetic batches split 3 + 2 and 4 + 1 (one row and unequal
counts: the split rule of the weight gradients depends on the row count).  Dropout is off unless a test says otherwise.

Bounds: "bit-equal" = the eight GPT-2 block matrices are torch.equal; "1e-6" = the whole flat buffer within 1e-6 of the reference's
norm (the project's bounds for the same kernels summed in another fp32 order: test_model_gpu.py's
test_trainer_gradients_equal_the_accumulating_path); 0.2 * lr absolute on parameters after one AdamW step
(test_fused_train_step_f32_vs_golden)."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_case  # noqa: E402
from mmtg_amd import MMTG, synth  # noqa: E402
from mmtg_amd.trainer import MMTGTrainer  # noqa: E402

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ["bf16", "bf16x3f", "bf16x3", "f32"]
SPLITS = [(3, 2), (4, 1)]
BLOCK_KEYS = ["decoder.gpt2.transformer.h.%d.%s" % (l, w) for l in range(2)
              for w in ("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")]


@functools.lru_cache(maxsize=None)
def _case():
    fx, meta, mcfg, gcfg, dcfg, weights, table, _ = load_case("tiny_s5")
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    return meta, mcfg, gcfg, dcfg, sd, table


def build(mode, pdrop=0.0):
    """tiny_s5's model; pdrop > 0 = the same weights with GPT-2's three dropouts on, in training mode."""
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


def part(lo, hi, seed=7):
    return {k: v[lo:hi] for k, v in rows5(seed).items()}


def assert_same_gradient(eng, got, ref, what=""):
    """bit-equal on the block matrices, 1e-6 of the reference's norm on the buffer"""
    rel = float((got.double() - ref.double()).norm() / ref.double().norm())
    print("%s: |got - ref| / |ref| = %.3e" % (what, rel))
    assert rel < 1e-6, (what, rel)
    for key in BLOCK_KEYS:
        a, b = eng.layout.view(got, key), eng.layout.view(ref, key)
        assert torch.equal(a, b) and float(a.abs().max()) > 0, (what, key)


# ---- 1
@pytest.mark.parametrize("mode", MODES)
def test_one_accumulation_step_is_today_s_trainer(mode):
    """accumulation_steps=1 and the keyword left out: three steps with dropout on from equal drop_seed leave equal bits in the
    master parameters after every step."""
    trs = []
    for kw in ({"accumulation_steps": 1}, {}):
        tr = MMTGTrainer(build(mode, 0.1), lr=1e-3, alpha=0.2, **kw)
        tr.eng.drop_seed = 4242
        trs.append(tr)
    for step in range(3):
        b = part(0, 5) if step != 1 else part(0, 3)
        outs = [tr.step(b, stage=3) for tr in trs]
        assert torch.equal(trs[0].eng.master, trs[1].eng.master), (mode, step, int((trs[0].eng.master != trs[1].eng.master).sum()))
        assert torch.equal(outs[0]["loss"], outs[1]["loss"])
        assert trs[0].micro_step == 0 and trs[0].sched_step == trs[0].eng.step_count == step + 1
    assert float((trs[0].eng.master - build(mode).engine().master).abs().max()) > 1e-4       # the steps really moved the parameters


# ---- 2
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "%d+%d" % s)
@pytest.mark.parametrize("mode", MODES)
def test_a_window_is_the_sum_of_its_micro_batches(mode, split):
    nA, nB = split
    A, B = part(0, nA), part(nA, 5)
    plain = MMTGTrainer(build(mode), lr=0.0, alpha=0.2)
    oA = plain.step(A, stage=3)
    gA, lA = plain.eng.grad.clone(), float(oA["loss"])
    oB = plain.step(B, stage=3)
    gB, lB = plain.eng.grad.clone(), float(oB["loss"])
    tr = MMTGTrainer(build(mode), lr=0.0, alpha=0.2, accumulation_steps=2)
    eng = tr.eng
    o1 = tr.step(A, stage=3)
    assert_same_gradient(eng, eng.grad, gA, "first call vs a plain step on A")
    assert tr.micro_step == 1 and eng.step_count == 0 and tr.sched_step == 0 and tr.window is None
    assert float(o1["loss"]) == pytest.approx(lA, rel=1e-6)
    o2 = tr.step(B, stage=3)
    assert float(o2["loss"]) == pytest.approx(lB, rel=1e-6)             # each call returns its own rows' scalars
    ref = gA.double() + gB.double()
    rel = float((eng.grad.double() - ref).norm() / ref.norm())
    print("window vs gA + gB: %.3e" % rel)
    assert rel < 1e-6, rel
    assert tr.micro_step == 0 and eng.step_count == 1 and tr.sched_step == 1
    assert float(tr._count.item()) == 5.0
    gn, gn_ref = float(tr.grad_norm()), float(ref.norm()) / 5
    assert abs(gn - gn_ref) <= 1e-5 * gn_ref, (gn, gn_ref)
    w = tr.window
    assert w["rows"] == 5 and isinstance(w["rows"], int)
    l_ref = (nA * lA + nB * lB) / 5
    assert abs(float(w["loss"]) - l_ref) <= 1e-6 * abs(l_ref), (float(w["loss"]), l_ref)
    assert torch.isfinite(w["lm_loss"]) and torch.isfinite(w["kl"])


# ---- 3
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_a_window_is_the_big_batch(mode):
    """k = 2 over 3 + 2 rows against one plain step on the five rows: the gradient within the bound of
    test_full_size_gradient_is_additive_over_row_shards, the parameters after the step within 0.2 * lr."""
    lr = 1e-3
    big = MMTGTrainer(build(mode), lr=lr, alpha=0.2)
    big.step(part(0, 5), stage=3)
    tr = MMTGTrainer(build(mode), lr=lr, alpha=0.2, accumulation_steps=2)
    tr.step(part(0, 3), stage=3)
    tr.step(part(3, 5), stage=3)
    g, ref = tr.eng.grad, big.eng.grad
    cos = float(torch.nn.functional.cosine_similarity(g, ref, dim=0))
    rel = float((g - ref).norm() / ref.norm())
    dp = float((tr.eng.master - big.eng.master).abs().max())
    print("cos %.7f rel %.3e max parameter difference %.3e" % (cos, rel, dp))
    assert cos > 0.99999 and rel < 2e-3, (cos, rel)
    assert dp <= 0.2 * lr, dp
    assert float((big.eng.master - build(mode).engine().master).abs().max()) > 0.5 * lr         # the step moved them by about lr
    assert float(tr._count.item()) == float(big._count.item()) == 5.0


# ---- 4
def test_zeroing_happens_once_and_the_lazy_list_holds():
    """Three windows of the same two micro-batches; the buffer is poisoned before the third, whose zero_grad uses the lazy list of the
    window's FIRST micro-batch's shape: finite afterwards and equal to the second window's gradient."""
    tr = MMTGTrainer(build("bf16"), lr=0.0, alpha=0.2, accumulation_steps=2)
    eng = tr.eng
    A, B = part(0, 3), part(3, 5)
    second = None
    for window in range(3):
        if window == 2:
            second = eng.grad.clone()
            eng.grad.fill_(1e30)            # anything left un-zeroed AND un-overwritten would show
        tr.step(A, stage=3)
        tr.step(B, stage=3)
    torch.cuda.synchronize()
    assert torch.isfinite(eng.grad).all()
    assert_same_gradient(eng, eng.grad, second, "third window (poisoned) vs second")
    assert len(eng._ow_desc) == 1 and next(iter(eng._ow_desc)) == (3, int(A["targets"].shape[1]))
    assert tr.sched_step == 3


# ---- 5
def test_the_stage_filter_inside_a_window():
    A, B = dict(part(0, 3)), dict(part(3, 5))
    A["rating"] = torch.tensor([1, 3, 5], device=DEV)           # stage 1 keeps two rows of A
    B["rating"] = torch.tensor([3, 2], device=DEV)              # and none of B
    plain = MMTGTrainer(build("bf16"), lr=0.0, alpha=0.2)
    plain.step(A, stage=1)
    ref = plain.eng.grad.clone()
    tr = MMTGTrainer(build("bf16"), lr=1e-3, alpha=0.2, accumulation_steps=2)
    eng = tr.eng
    o1 = tr.step(A, stage=1)
    assert o1 is not None and torch.isfinite(o1["loss"]) and tr.micro_step == 1
    assert tr.step(B, stage=1) is None
    assert tr.micro_step == 0 and tr.sched_step == 1 and eng.step_count == 1
    assert float(tr._count.item()) == 2.0 and tr.window["rows"] == 2
    assert_same_gradient(eng, eng.grad, ref, "A then an emptied B vs a plain stage-1 step on A")
    # a window of B twice: nothing moves
    before = eng.master.clone()
    assert tr.step(B, stage=1) is None and tr.micro_step == 1
    assert tr.step(B, stage=1) is None and tr.micro_step == 0
    assert torch.equal(eng.master, before) and eng.step_count == 1 and tr.sched_step == 1


# ---- 6
def test_flush_closes_a_partial_window():
    A, B = part(0, 3), part(3, 5)
    full = MMTGTrainer(build("bf16"), lr=1e-3, alpha=0.2, accumulation_steps=2)
    full.step(A, stage=3)
    full.step(B, stage=3)
    tr = MMTGTrainer(build("bf16"), lr=1e-3, alpha=0.2, accumulation_steps=4)
    assert tr.flush() is False
    tr.step(A, stage=3)
    tr.step(B, stage=3)
    assert tr.micro_step == 2 and tr.eng.step_count == 0
    assert tr.flush() is True
    assert tr.micro_step == 0 and tr.eng.step_count == 1 and tr.sched_step == 1 and tr.flush() is False
    assert float(tr._count.item()) == float(full._count.item()) == 5.0 and tr.window["rows"] == 5
    assert_same_gradient(tr.eng, tr.eng.grad, full.eng.grad, "flushed k = 4 window vs a k = 2 window")
    rel = float((tr.eng.master - full.eng.master).norm() / full.eng.master.norm())
    assert rel < 1e-6, rel
    assert float((tr.eng.master - build("bf16").engine().master).abs().max()) > 1e-4


# ---- 7
def test_resume_at_a_window_boundary():
    """bf16, dropout on, k = 2: two windows, checkpoint, one more window -- and a fresh model and trainer that load the checkpoint and
    run that window hold the same bits in the parameters and both moments."""
    A, B = part(0, 3), part(3, 5)
    model = build("bf16", 0.1)
    tr = MMTGTrainer(model, lr=1e-3, alpha=0.2, warmup_steps=2, total_steps=10, accumulation_steps=2)
    tr.eng.drop_seed = 4242
    for _ in range(2):
        tr.step(A, stage=3)
        tr.step(B, stage=3)
    sd_t = tr.state_dict()
    sd_m = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert sd_t["hparams"]["accumulation_steps"] == 2 and sd_t["sched_step"] == 2 and sd_t["step_count"] == 2
    tr.step(A, stage=3)
    with pytest.raises(RuntimeError, match=r"micro_step.*flush\(\)"):
        tr.state_dict()
    tr.step(B, stage=3)
    model2 = build("bf16", 0.1)
    model2.load_state_dict(sd_m)
    tr2 = MMTGTrainer(model2, lr=1e-3, alpha=0.2, warmup_steps=2, total_steps=10, accumulation_steps=2)
    tr2.load_state_dict(sd_t)
    assert tr2.current_lr() == pytest.approx(1e-3) and tr2.micro_step == 0
    tr2.step(A, stage=3)
    tr2.step(B, stage=3)
    for name in ("master", "opt_m", "opt_v"):
        a, b = getattr(tr.eng, name), getattr(tr2.eng, name)
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert tr.eng.step_count == tr2.eng.step_count == 3


# ---- 8
def test_a_host_exception_abandons_the_window_and_leaves_the_engine_clean(monkeypatch):
    """A Python exception (before any launch, no device fault) from the attention backward's launch wrapper, in the middle of the second
    micro-step's decoder backward -- column sums queued, deferral on.  Afterwards the trainer is at a boundary, the engine holds no
    queued sums, no side stream and no deferral, and the next full window's gradient is a fresh trainer's."""
    from mmtg_amd import engine as E
    A, B = part(0, 3), part(3, 5)
    tr = MMTGTrainer(build("bf16"), lr=0.0, alpha=0.2, accumulation_steps=2)
    eng = tr.eng
    orig = E.hip.attn_bwd
    state = {"armed": False, "seen": None}

    def failing(*a, **k):
        if state["armed"]:
            state["armed"] = False
            state["seen"] = (len(eng._sums), eng._defer)
            raise RuntimeError("host-side failure before the launch")
        return orig(*a, **k)

    monkeypatch.setattr(E.hip, "attn_bwd", failing)
    tr.step(A, stage=3)
    state["armed"] = True
    with pytest.raises(RuntimeError, match="host-side failure"):
        tr.step(B, stage=3)
    monkeypatch.setattr(E.hip, "attn_bwd", orig)
    assert state["seen"] is not None and state["seen"][0] > 0 and state["seen"][1] is True      # it struck mid-way
    assert tr.micro_step == 0
    assert eng._sums == [] and eng._tail_side is None and eng._defer is False and eng._tail_jobs == [] and eng._lazy is None
    assert eng.wgrad_overwrite is False and eng.step_count == 0 and tr.sched_step == 0
    tr.step(A, stage=3)
    tr.step(B, stage=3)
    fresh = MMTGTrainer(build("bf16"), lr=0.0, alpha=0.2, accumulation_steps=2)
    fresh.step(A, stage=3)
    fresh.step(B, stage=3)
    assert_same_gradient(eng, eng.grad, fresh.eng.grad, "the window after the exception vs a fresh trainer's")
    assert float(tr._count.item()) == 5.0 and eng.step_count == 1


# ---- 9
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_the_exchange_runs_once_per_window(tmp_path):
    """WORLD_SIZE=1, MMTG_FORCE_DDP=1, k = 3, two windows of 3 + 1 + 2 rows with dropout on, in a fresh child process: the row count and
    every gradient bucket go through RCCL all-reduces in the CLOSING call of each window and nowhere else, the bucket hook is installed
    for the closing backward alone, and the parameters equal a non-distributed k = 3 trainer's bit for bit."""
    out = str(tmp_path / "acc")
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0", MMTG_FORCE_DDP="1")
    p = subprocess.Popen([sys.executable, os.path.join(HERE, "accum_ddp_worker.py"), out], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        log, _ = p.communicate(timeout=600)
    except subprocess.TimeoutExpired:
        p.kill()
        log, _ = p.communicate()
    assert p.returncode == 0, log[-4000:]
    res = torch.load(out + ".r0", weights_only=False)
    assert res.get("ok") and res["backend"] == "nccl"
    per_call = res["per_call"]
    assert len(per_call) == 6
    for call, elems in enumerate(per_call):
        if call % 3 != 2:
            assert elems == [], (call, elems)
        else:
            assert len(elems) == res["buckets"] + 1 and elems[0] == 1 and sum(elems[1:]) == res["layout_total"], (call, elems)
    assert res["hooks"] == [False, False, True] * 2
    assert res["count"] == 6.0
    for window in range(2):
        a, b = res["params"][True][window], res["params"][False][window]
        assert torch.equal(a, b), (window, int((a != b).sum()), float((a - b).abs().max()))
    assert float((res["params"][True][0] - res["params"][True][1]).abs().max()) > 1e-4
