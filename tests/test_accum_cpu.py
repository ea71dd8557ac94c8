"""Gradient accumulation, the trainer's host side (MMTGTrainer(accumulation_steps=k)): no GPU.

A stand-in engine records what the trainer calls and with which `wgrad_overwrite` / `bucket_hook` at that moment;
tests/test_accum_gpu.py holds the real engine's gradients to the rule."""
import types

import pytest
import torch

from mmtg_amd.configs import gpt2_config, make_model_cfgs
from mmtg_amd.engine import ParamLayout
from mmtg_amd.trainer import MMTGTrainer, linear_schedule

T = 7


@pytest.fixture(scope="module")
def layout():
    return ParamLayout(make_model_cfgs(seq_len=5), gpt2_config(n_layer=2, vocab_size=160, n_positions=256))


class StandInEngine:
    """Records (name, ...) per call.  `fail_backward` = the 1-based backward call that raises."""

    def __init__(self, layout, fail_backward=None):
        self.layout, self.dev = layout, torch.device("cpu")
        self.opt_m = self.opt_v = None
        self.step_count, self.drop_seed = 0, 5
        self.grad = torch.zeros(4)
        self.wgrad_overwrite, self.bucket_hook, self._ow_rec = False, None, None
        self.act = {}
        self.calls, self.backwards, self.fail_backward = [], 0, fail_backward

    def zero_grad(self, shape_key=None):
        self.calls.append(("zero_grad", shape_key))

    def forward(self, batch, **kw):
        n = int(batch["targets"].shape[0])
        self.calls.append(("forward", n))
        self.act = {"T": int(batch["targets"].shape[1]), "kl": torch.tensor([0.5 * n])}

    def loss(self, ratings, stage, batch_den=None):
        self.calls.append(("loss", batch_den))
        return torch.tensor([float(batch_den), 10.0 * batch_den])

    def loss_backward(self, gscale, lm_coef=0.0):
        self.calls.append(("loss_backward", gscale))
        return "dl"

    def backward(self, dl, dkl=0.0):
        self.backwards += 1
        self.calls.append(("backward", self.wgrad_overwrite, self.bucket_hook))
        if self.backwards == self.fail_backward:
            raise RuntimeError("stand-in backward failed")

    def _finish_overwrite_record(self):
        self.calls.append(("_finish_overwrite_record",))

    def adamw_step(self, lr, max_norm, betas, eps, wd, count=None, groups=None):
        self.step_count += 1
        self.calls.append(("adamw_step", lr, float(count[0])))

    def names(self):
        return [c[0] for c in self.calls]


def make(layout, fail_backward=None, **kw):
    eng = StandInEngine(layout, fail_backward)
    model = types.SimpleNamespace(engine=lambda: eng, training=False)
    return MMTGTrainer(model, **kw), eng


def batch(ratings):
    n = len(ratings)
    return {"rating": torch.tensor(ratings, dtype=torch.long), "targets": torch.zeros(n, T, dtype=torch.long)}


MICRO = ["forward", "loss", "loss_backward", "backward"]


def test_call_order_of_a_window(layout):
    tr, eng = make(layout, lr=1e-3, alpha=0.5, accumulation_steps=3)
    outs, seen = [], []
    for rows in (3, 2, 1):
        outs.append(tr.step(batch([3] * rows)))
        seen.append((tr.micro_step, tr.sched_step, eng.step_count))
    assert seen == [(1, 0, 0), (2, 0, 0), (0, 1, 1)]
    assert eng.names() == (["zero_grad"] + MICRO + ["_finish_overwrite_record"] + MICRO + MICRO + ["adamw_step"])
    assert [c for c in eng.calls if c[0] == "zero_grad"] == [("zero_grad", (3, T))]
    assert [c[1] for c in eng.calls if c[0] == "backward"] == [True, False, False]
    assert all(c[2] is None for c in eng.calls if c[0] == "backward")            # no reducer: no hook
    assert [c[1] for c in eng.calls if c[0] == "forward"] == [3, 2, 1]
    assert [c[1] for c in eng.calls if c[0] == "loss"] == [3, 2, 1]             # each micro-batch's own row count: a row SUM
    assert [c[1] for c in eng.calls if c[0] == "loss_backward"] == [3.0, 2.0, 1.0]
    assert eng.calls[-1] == ("adamw_step", 1e-3, 6.0)                             # the window's rows, filled once
    assert eng.wgrad_overwrite is False
    # every call returns its own rows' scalars; the window holds the row-weighted mean
    assert [float(o["loss"]) for o in outs] == [3.0, 2.0, 1.0]
    w = tr.window
    assert w["rows"] == 6 and isinstance(w["rows"], int)
    assert float(w["loss"]) == pytest.approx((9 + 4 + 1) / 6, rel=1e-6)
    assert float(w["lm_loss"]) == pytest.approx(10 * (9 + 4 + 1) / 6, rel=1e-6)
    assert float(w["kl"]) == pytest.approx(0.5 * (9 + 4 + 1) / 6, rel=1e-6)
    # the next window zeroes again, with ITS first micro-batch's shape
    tr.step(batch([3, 3]))
    assert eng.calls[-6][:2] == ("zero_grad", (2, T)) and eng.calls[-2][:2] == ("backward", True) and tr.micro_step == 1


def test_the_default_is_the_single_step(layout):
    tr, eng = make(layout, lr=1e-3)
    assert tr.accumulation_steps == 1 and tr.window is None
    for i in range(2):
        out = tr.step(batch([3, 3]))
        assert (tr.micro_step, tr.sched_step, eng.step_count) == (0, i + 1, i + 1)
        assert tr.window["rows"] == 2 and tr.window["loss"] is out["loss"]
    assert eng.names() == 2 * (["zero_grad"] + MICRO + ["_finish_overwrite_record", "adamw_step"])
    assert [c[1] for c in eng.calls if c[0] == "backward"] == [True, True]
    assert tr.flush() is False


def test_the_schedule_counts_windows(layout):
    tr, eng = make(layout, lr=1.0, warmup_steps=2, total_steps=10, accumulation_steps=2)
    lrs = []
    for call in range(8):
        lrs.append(tr.current_lr())
        tr.step(batch([3]))
        assert tr.sched_step == (call + 1) // 2
    assert lrs == [linear_schedule(c // 2, 2, 10) for c in range(8)]            # constant inside a window
    assert [c[1] for c in eng.calls if c[0] == "adamw_step"] == [linear_schedule(w, 2, 10) for w in range(4)]


def test_flush_closes_a_partial_window(layout):
    tr, eng = make(layout, accumulation_steps=4)
    assert tr.flush() is False and eng.calls == []
    tr.step(batch([3, 3]))
    assert tr.micro_step == 1
    assert tr.flush() is True
    assert eng.calls[-1][0] == "adamw_step" and eng.calls[-1][2] == 2.0
    assert (tr.micro_step, tr.sched_step, eng.step_count, tr.window["rows"]) == (0, 1, 1, 2)
    assert float(tr.window["loss"]) == 2.0
    assert tr.flush() is False and eng.names().count("adamw_step") == 1
    tr.step(batch([3]))
    assert eng.calls[-6][:2] == ("zero_grad", (1, T))                            # a fresh window after the flush


def test_empty_micro_batches_count_as_calls(layout):
    tr, eng = make(layout, accumulation_steps=2)
    # stage 1 keeps ratings < 2 and > 4: nothing of the second micro-batch
    assert tr.step(batch([1, 3, 5]), stage=1) is not None
    n = len(eng.calls)
    assert tr.step(batch([3, 3]), stage=1) is None
    assert eng.names()[n:] == ["adamw_step"] and eng.calls[-1][2] == 2.0        # no forward, and the window closed on time
    assert (tr.micro_step, tr.sched_step, tr.window["rows"]) == (0, 1, 2)
    # the other way round: the window's first BACKWARD is the second call's, and it is the one that zeroes and overwrites
    n = len(eng.calls)
    assert tr.step(batch([3]), stage=1) is None and len(eng.calls) == n and tr.micro_step == 1
    assert tr.step(batch([5]), stage=1) is not None
    assert eng.names()[n:] == ["zero_grad"] + MICRO + ["_finish_overwrite_record", "adamw_step"]
    assert eng.calls[n + 4][1] is True and tr.sched_step == 2
    # a window of only empty calls: no optimizer step, no counter moves
    n, w = len(eng.calls), tr.window
    assert tr.step(batch([3]), stage=1) is None and tr.micro_step == 1
    assert tr.step(batch([2, 4]), stage=1) is None and tr.micro_step == 0
    assert len(eng.calls) == n and tr.sched_step == 2 and eng.step_count == 2 and tr.window is w


def test_checkpoints_only_at_a_boundary(layout):
    tr, eng = make(layout, accumulation_steps=2)
    assert tr.state_dict()["hparams"]["accumulation_steps"] == 2
    tr.step(batch([3]))
    with pytest.raises(RuntimeError, match=r"micro_step.*flush\(\)"):
        tr.state_dict()
    tr.step(batch([3]))
    sd = tr.state_dict()
    assert sd["hparams"]["accumulation_steps"] == 2 and sd["sched_step"] == 1
    other, _ = make(layout, accumulation_steps=3)
    other.load_state_dict(sd)
    assert other.accumulation_steps == 3 and other.sched_step == 1
    assert other.state_dict()["hparams"]["accumulation_steps"] == 3


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2"])
def test_accumulation_steps_is_validated(layout, bad):
    with pytest.raises(ValueError, match=repr(bad).replace(".", r"\.")):
        make(layout, accumulation_steps=bad)


def test_an_exception_abandons_the_window(layout):
    tr, eng = make(layout, fail_backward=2, accumulation_steps=3)
    tr.step(batch([3, 3]))
    with pytest.raises(RuntimeError, match="stand-in backward failed"):
        tr.step(batch([3]))
    assert tr.micro_step == 0 and eng.wgrad_overwrite is False and tr.sched_step == 0
    n = len(eng.calls)
    tr.step(batch([3, 3, 3]))
    assert eng.calls[n][:2] == ("zero_grad", (3, T)) and eng.calls[-2][:2] == ("backward", True) and tr.micro_step == 1
    tr.reset_window()
    assert tr.micro_step == 0
    tr.step(batch([3]))
    assert eng.calls[-6][:2] == ("zero_grad", (1, T)) and tr.flush() is True
    assert eng.calls[-1][0] == "adamw_step" and eng.calls[-1][2] == 1.0


def test_the_bucket_hook_is_installed_for_the_closing_backward_only(layout):
    """With a reducer (stand-in: not active, as a single process without a process group) the hook is the trainer's during the
    closing micro-step's backward and None during the others; flush() after a hook-less backward still steps."""
    tr, eng = make(layout, accumulation_steps=3, distributed=True)
    assert tr.reducer is not None and not tr.reducer.active and eng.bucket_hook is None
    for rows in (2, 1, 2):
        tr.step(batch([3] * rows))
    hooks = [c[2] for c in eng.calls if c[0] == "backward"]
    assert hooks[0] is None and hooks[1] is None and callable(hooks[2])
    one, eng1 = make(layout, distributed=True)
    assert callable(eng1.bucket_hook)                 # k = 1: every backward closes
    one.step(batch([3]))
    assert callable([c[2] for c in eng1.calls if c[0] == "backward"][0])
