"""Weight averaging, the host side (mmtg_ema_update / mmtg_swap_f32's checks, the bound, MMTGTrainer(ema_decay=...)): no GPU.

A stand-in engine records what the trainer calls; tests/test_ema_ops_gpu.py holds the kernels and tests/test_ema_gpu.py the real
engine to the rule."""
import ctypes
import fnmatch
import os
import re
import types

import numpy as np
import pytest
import torch

from ema_ref import check_update, ema_restated32
from mmtg_amd import hip
from mmtg_amd.trainer import MMTGTrainer, save_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 7


# ---- 1
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    exports = open(os.path.join(ROOT, "mmtg_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    lib = ctypes.CDLL(hip.lib_path())
    for name in ("mmtg_ema_update", "mmtg_swap_f32"):
        assert name + "(" in header and name in hip.exported_symbols() and name in hip._SIGS and hasattr(lib, name)
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), (name, patterns)
    assert len(hip._SIGS["mmtg_ema_update"][0]) == 6 and len(hip._SIGS["mmtg_swap_f32"][0]) == 4
    assert hip.lib().mmtg_abi_version() == hip.ABI_VERSION == 12
    assert callable(hip.ema_update) and callable(hip.swap_f32)


# ---- 2
def test_arguments_are_checked_before_any_device_call():
    """fake device addresses: every case is refused on the host, so no GPU is touched"""
    L = hip.lib()
    a, b = 0x7000000000, 0x7100000000
    cases = {
        "null ema": (None, b, 100, 0.1), "null p": (a, None, 100, 0.1), "n = 0": (a, b, 0, 0.1), "n < 0": (a, b, -4, 0.1),
        "w = -0.1": (a, b, 100, -0.1), "w = 1.5": (a, b, 100, 1.5), "w = nan": (a, b, 100, float("nan")),
        "overlap": (a, a + 4 * 99, 100, 0.1), "overlap the other way": (a + 4 * 99, a, 100, 0.1), "same": (a, a, 100, 0.1),
    }
    for what, (ema, p, n, w) in cases.items():
        assert L.mmtg_ema_update(ema, p, n, w, None, None) != 0, what
        err = L.mmtg_last_error().decode()
        assert err.startswith("ema_update: "), (what, err)
    assert L.mmtg_ema_update(a, a + 4 * 99, 100, 0.1, None, None) != 0 and b"overlap" in L.mmtg_last_error()
    for what, (x, y, n) in {"overlap": (a, a + 4 * 99, 100), "overlap the other way": (a + 4 * 99, a, 100), "same": (a, a, 8),
                            "null a": (None, b, 8), "null b": (a, None, 8), "n = 0": (a, b, 0)}.items():
        assert L.mmtg_swap_f32(x, y, n, None) != 0, what
        err = L.mmtg_last_error().decode()
        assert err.startswith("swap_f32: "), (what, err)
    assert L.mmtg_swap_f32(a, a + 4 * 99, 100, None) != 0 and b"overlap" in L.mmtg_last_error()


# ---- 3
@pytest.mark.parametrize("w", [0.0, 1e-4, 1e-3, 0.1, 0.9, 1.0])
def test_the_bound_is_a_real_bound(w):
    """The float32 restatement of the update against the float64 formula: |e| about 1 and about 0.02, |p - e| from 1e-7 to 10, all
    normal-range floats.  It stays within the derived bound and returns e bit for bit where p == e."""
    rng = np.random.default_rng(1234)
    n = 20000
    for scale in (1.0, 0.02):
        e = (scale * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        mag = 10.0 ** rng.uniform(-7.0, 1.0, n)
        p = (e.astype(np.float64) + mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        e[97] = -0.0                                # (one of the elements planted next: checkpoints hold a -0 here and there)
        p[::97] = e[::97]
        got = ema_restated32(e, p, w)
        check_update(e, p, w, got, "w = %g, |e| ~ %g" % (w, scale))
        if w == 0.0:
            assert (got.view(np.int32) == e.view(np.int32)).all()


# ---- 4: the trainer on a stand-in engine
class Layout:
    """two tensors and a pad in a 24-element flat buffer"""
    total = 24
    entries = {"a.weight": (0, (2, 3), 6), "decoder.gpt2.transformer.wte.weight": (8, (4, 2), 8)}

    def view(self, flat, key):
        off, shape, n = self.entries[key]
        return flat[off:off + n].view(shape)


class PlainEngine:
    """Records (name, ...) per call; has nothing of the average: a trainer without ema_decay must not miss it."""

    def __init__(self):
        self.layout, self.dev = Layout(), torch.device("cpu")
        self.opt_m = self.opt_v = None
        self.step_count, self.drop_seed = 0, 5
        self.master = torch.arange(24, dtype=torch.float32)
        self.wgrad_overwrite, self.bucket_hook, self._ow_rec = False, None, None
        self.act, self.calls = {}, []

    def zero_grad(self, shape_key=None):
        self.calls.append(("zero_grad", shape_key))

    def forward(self, batch, **kw):
        n = int(batch["targets"].shape[0])
        self.calls.append(("forward", n))
        self.act = {"T": int(batch["targets"].shape[1]), "kl": torch.tensor([0.5 * n])}

    def loss(self, ratings, stage, batch_den=None):
        return torch.tensor([1.0, 10.0])

    def loss_backward(self, gscale, lm_coef=0.0):
        return "dl"

    def backward(self, dl, dkl=0.0):
        self.calls.append(("backward",))

    def _finish_overwrite_record(self):
        pass

    def adamw_step(self, lr, max_norm, betas, eps, wd, count=None, groups=None):
        self.step_count += 1
        self.master = self.master + 1.0
        self.calls.append(("adamw_step", float(count[0])))

    def names(self):
        return [c[0] for c in self.calls]


class EmaEngine(PlainEngine):
    def __init__(self):
        super().__init__()
        self.ema = None

    def ema_init(self):
        if self.ema is None:
            self.calls.append(("ema_init", self.step_count))
            self.ema = self.master.clone()

    def ema_update(self, w, count=None):
        self.ema_init()
        self.calls.append(("ema_update", w, float(count[0])))
        self.ema = self.ema + w * (self.master - self.ema)

    def swap_ema(self):
        self.calls.append(("swap_ema",))
        self.master, self.ema = self.ema, self.master


def make(engine=EmaEngine, **kw):
    eng = engine()
    sd = {"a.weight": torch.full((2, 3), -1.0), "decoder.gpt2.transformer.wte.weight": torch.full((4, 2), -2.0),
          "decoder.gpt2.lm_head.weight": torch.full((4, 2), -2.0), "other.buffer": torch.tensor([7, 8])}
    model = types.SimpleNamespace(engine=lambda: eng, training=False, state_dict=lambda: sd, eval=lambda: None, train=lambda mode=True: None)
    return MMTGTrainer(model, **kw), eng


def batch(rows=2):
    return {"rating": torch.full((rows,), 3, dtype=torch.long), "targets": torch.zeros(rows, T, dtype=torch.long)}


@pytest.mark.parametrize("warmup", [True, False])
def test_the_decay_schedule(warmup):
    decay = 0.9
    tr, eng = make(lr=1e-3, ema_decay=decay, ema_warmup=warmup)
    for _ in range(12):
        tr.step(batch())
    ws = [c[1] for c in eng.calls if c[0] == "ema_update"]
    want = [1.0 - (min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay) for t in range(12)]
    assert ws == want                                        # equal doubles
    assert warmup == (ws[0] == 0.9) and (ws[-1] == 1.0 - 0.9) != warmup and tr.ema_updates == 12
    assert [c[2] for c in eng.calls if c[0] == "ema_update"] == [2.0] * 12           # the count AdamW was given


def test_one_update_per_window_after_the_step():
    tr, eng = make(lr=1e-3, ema_decay=0.99, accumulation_steps=3)
    for i in range(3):
        assert tr.ema_updates == 0
        tr.step(batch())
    assert tr.ema_updates == 1
    tail = [n for n in eng.names() if n in ("ema_init", "adamw_step", "ema_update")]
    assert tail == ["ema_init", "adamw_step", "ema_update"]         # the first copy BEFORE the first step, the update after it
    assert ("ema_init", 0) in eng.calls
    tr.step(batch())
    assert tr.ema_updates == 1 and eng.names().count("ema_update") == 1          # a micro-step moves nothing
    assert tr.flush() is True
    assert tr.ema_updates == 2 and eng.names()[-2:] == ["adamw_step", "ema_update"] and eng.names().count("ema_init") == 1
    # an all-empty single-rank window never reaches the step: no update either
    for _ in range(3):
        assert tr.step(batch(), stage=1) is None
    assert tr.ema_updates == 2 and eng.names().count("ema_update") == 2


def test_without_a_decay_the_engine_is_not_asked():
    tr, eng = make(PlainEngine, lr=1e-3)
    assert tr.ema_decay is None
    tr.step(batch())
    sd = tr.state_dict()
    assert sd["ema"] is None and sd["hparams"]["ema_decay"] is None and sd["hparams"]["ema_warmup"] is True
    tr.load_state_dict(dict(sd, ema={"decay": 0.9, "warmup": True, "updates": 3, "average": torch.zeros(24)}))      # ignored
    assert tr.evaluate([]) == (0.0, 0.0)
    assert not hasattr(eng, "ema") and eng.names() == ["zero_grad", "forward", "backward", "adamw_step"]
    for call in (tr.ema_state_dict, lambda: tr.averaged_weights().__enter__(), lambda: tr.evaluate([], averaged=True),
                 lambda: save_checkpoint(os.devnull, tr.model, tr, averaged=True)):
        with pytest.raises(RuntimeError, match="ema_decay=None"):
            call()
    with pytest.raises(RuntimeError, match="needs the trainer"):
        save_checkpoint(os.devnull, tr.model, averaged=True)
    assert not hasattr(eng, "ema")


@pytest.mark.parametrize("bad", [0, 1, -1, "x", 0.0, 1.0, True, float("nan")])
def test_the_decay_is_validated(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        make(ema_decay=bad)


def test_state_dict_round_trip():
    tr, eng = make(lr=1e-3, ema_decay=0.9, ema_warmup=False)
    sd0 = tr.state_dict()
    assert sd0["format"] == "mmtg-trainer-1"
    assert sd0["ema"] == {"decay": 0.9, "warmup": False, "updates": 0, "average": None}
    assert sd0["hparams"]["ema_decay"] == 0.9 and sd0["hparams"]["ema_warmup"] is False
    with pytest.raises(RuntimeError, match="no optimizer step"):
        tr.ema_state_dict()
    for _ in range(3):
        tr.step(batch())
    sd = tr.state_dict()
    avg = sd["ema"]["average"]
    assert sd["ema"]["updates"] == 3 and avg.dtype == torch.float32 and avg.shape == (24,) and avg.device.type == "cpu"
    assert torch.equal(avg, eng.ema) and avg.data_ptr() != eng.ema.data_ptr()
    other, oeng = make(lr=1e-3, ema_decay=0.5)
    other.load_state_dict(sd)
    assert torch.equal(oeng.ema, eng.ema) and oeng.ema.data_ptr() != avg.data_ptr() and other.ema_updates == 3
    assert other.ema_decay == 0.5 and other.ema_warmup is True                   # the trainer's own, like lr
    # a dict without an average (an older checkpoint, a run that kept none, a run that had not stepped) resets both
    for old in ({k: v for k, v in sd.items() if k != "ema"}, dict(sd, ema=None), dict(sd, ema=sd0["ema"])):
        other.load_state_dict(sd)
        other.load_state_dict(old)
        assert oeng.ema is None and other.ema_updates == 0
    other.step(batch())
    assert oeng.names()[-3:] == ["ema_init", "adamw_step", "ema_update"] and other.ema_updates == 1      # ... and restarts at the next step
    with pytest.raises(ValueError, match="average of 23 elements"):
        other.load_state_dict(dict(sd, ema=dict(sd["ema"], average=torch.zeros(23))))


def test_ema_state_dict_takes_the_flat_keys_from_the_average():
    tr, eng = make(lr=1e-3, ema_decay=0.9)
    tr.step(batch())
    out = tr.ema_state_dict()
    model_sd = tr.model.state_dict()
    assert list(out) == list(model_sd)
    for k, v in out.items():
        assert v.shape == model_sd[k].shape and v.dtype == model_sd[k].dtype and v.device.type == "cpu"
    assert torch.equal(out["a.weight"], eng.ema[0:6].view(2, 3))
    assert torch.equal(out["decoder.gpt2.transformer.wte.weight"], eng.ema[8:16].view(4, 2))
    assert torch.equal(out["decoder.gpt2.lm_head.weight"], eng.ema[8:16].view(4, 2))          # the tied head lives in the buffer too
    assert torch.equal(out["other.buffer"], torch.tensor([7, 8]))                             # anything else: the model's
    with tr.averaged_weights():
        inside = tr.ema_state_dict()                 # the average sits in the master now: still the average
    assert all(torch.equal(inside[k], out[k]) for k in out)


def test_the_context_refuses_what_would_mix_the_buffers():
    tr, eng = make(lr=1e-3, ema_decay=0.9, accumulation_steps=2)
    with pytest.raises(RuntimeError, match="no optimizer step"):
        with tr.averaged_weights():
            pass
    tr.step(batch())
    tr.step(batch())
    tr.step(batch())                                 # an open window: entering is allowed
    master, ema = eng.master.clone(), eng.ema.clone()
    n = len(eng.calls)
    with tr.averaged_weights() as inside:
        assert inside is tr and torch.equal(eng.master, ema) and torch.equal(eng.ema, master)
        for what, call in (("step()", lambda: tr.step(batch())), ("flush()", tr.flush), ("state_dict()", tr.state_dict),
                           ("load_state_dict()", lambda: tr.load_state_dict({})),
                           ("averaged_weights()", lambda: tr.averaged_weights().__enter__()),
                           ("averaged_weights()", lambda: tr.evaluate([], averaged=True))):
            with pytest.raises(RuntimeError, match=re.escape(what) + " inside averaged_weights"):
                call()
        assert tr.evaluate([]) == (0.0, 0.0)
    assert eng.names()[n:] == ["swap_ema", "swap_ema"] and tr.micro_step == 1          # nothing else ran, the window is still open
    assert torch.equal(eng.master, master) and torch.equal(eng.ema, ema)
    tr.step(batch())
    assert tr.ema_updates == 2


def test_the_context_swaps_back_when_its_body_raises():
    tr, eng = make(lr=1e-3, ema_decay=0.9)
    tr.step(batch())
    master = eng.master.clone()
    with pytest.raises(KeyError):
        with tr.averaged_weights():
            raise KeyError("body")
    assert eng.names()[-2:] == ["swap_ema", "swap_ema"] and torch.equal(eng.master, master)
    tr.step(batch())                                 # ... and the trainer works again
    n = len(eng.calls)
    tr.evaluate([], averaged=True)
    assert eng.names()[n:] == ["swap_ema", "swap_ema"]
