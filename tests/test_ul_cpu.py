"""Token-level unlikelihood on repeated lyric tokens, the host side: the three entries' declarations and argument checks, the trainer's
arguments and the calls it makes (on a stand-in engine), and the yardstick that shows the bounds of tests/ul_ref.py admit a float32
evaluation of the kernels' expressions on every case of tests/test_ul_ops_gpu.py.  No GPU."""
import ctypes
import fnmatch
import os
import re
import types

import pytest
import torch

import ul_ref as R
from mmtg_amd import hip
from mmtg_amd.trainer import MMTGTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmtg_loss_ul_fwd", "mmtg_loss_bwd_ul", "mmtg_loss_bwd_ul_x3")
T = 7


# ---- 1
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    exports = open(os.path.join(ROOT, "mmtg_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    lib = ctypes.CDLL(hip.lib_path())
    for name in ENTRIES:
        assert name + "(" in header and name in hip.exported_symbols() and name in hip._SIGS and hasattr(lib, name)
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), (name, patterns)
    assert [len(hip._SIGS[n][0]) for n in ENTRIES] == [17, 22, 21]
    assert hip.lib().mmtg_abi_version() == hip.ABI_VERSION == 12
    assert "#define MMTG_ABI_VERSION 12" in header and "MMTG_UL_FLOOR 1e-5f" in header
    assert callable(hip.loss_ul_fwd) and callable(hip.loss_bwd_ul) and callable(hip.loss_bwd_ul_x3)
    assert (hip.UL_FLOOR, hip.UL_MAX_EXCLUDE, hip.UL_MAX_L) == (1e-5, 32, 1024)


# ---- 2: fake device addresses: every case is refused on the host, so no GPU is touched
A = [0x7000000000 + 0x100000000 * i for i in range(12)]
NAN, INF = float("nan"), float("inf")


def _refused(fn, prefix, args, what, match=None):
    L = hip.lib()
    assert fn(*args) != 0, what
    err = L.mmtg_last_error().decode()
    assert err.startswith(prefix + ": "), (what, err)
    if match:
        assert match in err, (what, err)


def test_loss_ul_fwd_checks_its_arguments():
    fn = hip.lib().mmtg_loss_ul_fwd
    #       dtype logits ldl  V  targets lse  exclude n  B  P  L  den  ul_row S    sample ul   stream
    good = [0, A[0], 336, 333, A[1], A[2], A[3], 5, 2, 3, 66, 2.0, A[4], A[5], A[6], A[7], None]
    bad = {"dtype": (0, 7), "null logits": (1, None), "ldl < V": (2, 300), "V = 0": (3, 0), "null targets": (4, None), "null lse": (5, None),
           "null exclude with ids": (6, None), "n_exclude = -1": (7, -1), "n_exclude = 33": (7, 33), "B = 0": (8, 0), "P < 0": (9, -1),
           "L = 0": (10, 0), "L = 1025": (10, 1025), "batch_den = 0": (11, 0.0), "batch_den nan": (11, NAN), "batch_den inf": (11, INF),
           "null ul_row": (12, None), "null S": (13, None), "null ul_sample": (14, None), "null ul": (15, None)}
    for what, (i, v) in bad.items():
        args = list(good)
        args[i] = v
        _refused(fn, "loss_ul_fwd", args, what, "at most 1024" if what == "L = 1025" else None)


def test_loss_bwd_ul_checks_its_arguments():
    fn = hip.lib().mmtg_loss_bwd_ul
    #       dtype ldtype logits ldl V  topic targets lse coef gscale lm  S    u   exclude n  B  P  L  dlogits ldd Vpad stream
    good = [1, 0, A[0], 384, 333, A[1], A[2], A[3], A[4], 1.0, 0.1, A[5], 0.3, A[6], 5, 2, 3, 66, A[7], 384, 384, None]
    bad = {"dtype": (0, 5), "bf16 logits, fp32 out": ((0, 1), (0, 1)), "null logits": (2, None), "ldl < V": (3, 200), "V = 0": (4, 0),
           "null topic with lm rows": (5, None), "null targets": (6, None), "null lse": (7, None), "null coef": (8, None), "null S": (11, None),
           "u < 0": (12, -0.1), "u nan": (12, NAN), "u inf": (12, INF), "null exclude with ids": (13, None), "n_exclude = -1": (14, -1),
           "n_exclude = 33": (14, 33), "B = 0": (15, 0), "P < 0": (16, -2), "L = 0": (17, 0), "L = 1025": (17, 1025), "null dlogits": (18, None),
           "ldd < Vpad": (19, 376), "Vpad < V": (20, 328), "in place across types": ((18,), (A[0],)),
           "in place across strides": ((1, 18, 19), (1, A[0], 392)), "misaligned logits": (2, A[0] + 4), "misaligned dlogits": (18, A[7] + 2)}
    for what, (i, v) in bad.items():
        args = list(good)
        for k, val in zip(i if isinstance(i, tuple) else (i,), v if isinstance(i, tuple) else (v,)):
            args[k] = val
        _refused(fn, "loss_bwd_ul", args, what, "in-place" if what.startswith("in place") else None)


def test_loss_bwd_ul_x3_checks_its_arguments():
    fn = hip.lib().mmtg_loss_bwd_ul_x3
    M, ld = 2 * 69, 384
    #       logits ldl V   topic targets lse  coef gscale lm  S     u   exclude n  B  P  L  planes ldd plane  Vpad stream
    good = [A[0], ld, 333, A[1], A[2], A[3], A[4], 1.0, 0.1, A[5], 0.3, A[6], 5, 2, 3, 66, A[7], ld, M * ld, 384, None]
    bad = {"null logits": (0, None), "ldl % 4": (1, 386), "ldl < Vpad": (1, 380), "V = 0": (2, 0), "null topic with lm rows": (3, None),
           "null targets": (4, None), "null lse": (5, None), "null coef": (6, None), "null S": (9, None), "u < 0": (10, -1.0), "u nan": (10, NAN),
           "u inf": (10, INF), "null exclude with ids": (11, None), "n_exclude = -1": (12, -1), "n_exclude = 33": (12, 33), "B = 0": (13, 0),
           "L = 1025": (15, 1025), "null planes": (16, None), "misaligned planes": (16, A[7] + 8), "ldd % 8": (17, 388), "lo plane in front": (18, -M * ld),
           "planes overlap": (18, (M - 1) * ld), "plane % 8": (18, M * ld + 4), "Vpad % 8": (19, 380)}
    for what, (i, v) in bad.items():
        args = list(good)
        args[i] = v
        _refused(fn, "loss_bwd_ul_x3", args, what, "lo plane" if what in ("lo plane in front", "planes overlap", "plane % 8") else None)


# ---- 3: the trainer on a stand-in engine
class Layout:
    total = 24
    entries = {"a.weight": (0, (2, 3), 6)}


class PlainEngine:
    """today's engine surface, nothing of the term: a trainer with ul_weight = 0 must not miss it"""

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
        self.act = {"T": int(batch["targets"].shape[1]) + 2, "kl": torch.tensor([0.5 * n])}

    def loss(self, ratings, stage, batch_den=None):
        self.calls.append(("loss", stage, batch_den))
        return torch.tensor([1.0, 10.0])

    def loss_backward(self, gscale, lm_coef=0.0):
        self.calls.append(("loss_backward", gscale, lm_coef))
        return "dl"

    def backward(self, dl, dkl=0.0):
        self.calls.append(("backward", dl))

    def _finish_overwrite_record(self):
        pass

    def adamw_step(self, lr, max_norm, betas, eps, wd, count=None, groups=None):
        self.step_count += 1
        self.calls.append(("adamw_step", float(count[0])))

    def names(self):
        return [c[0] for c in self.calls]


class UlEngine(PlainEngine):
    def set_ul_exclude(self, ids):
        self.calls.append(("set_ul_exclude", tuple(ids)))

    def ul_loss(self, batch_den=None):
        self.calls.append(("ul_loss", batch_den))
        return torch.tensor([0.25 * batch_den if batch_den else 3.0])

    def loss_backward_ul(self, gscale, lm_coef=0.0, ul_coef=0.0):
        self.calls.append(("loss_backward_ul", gscale, lm_coef, ul_coef))
        return "dl_ul"


def make(engine=UlEngine, **kw):
    eng = engine()
    model = types.SimpleNamespace(engine=lambda: eng, training=False, state_dict=lambda: {}, eval=lambda: None, train=lambda mode=True: None)
    return MMTGTrainer(model, **kw), eng


def batch(rows=2):
    return {"rating": torch.full((rows,), 3, dtype=torch.long), "targets": torch.zeros(rows, T, dtype=torch.long)}


@pytest.mark.parametrize("kw", [{}, {"ul_weight": 0.0}, {"ul_weight": 0, "ul_exclude_ids": (5, 6)}])
def test_without_a_weight_the_trainer_makes_today_s_calls(kw):
    tr, eng = make(PlainEngine, lr=1e-3, lm_weight=0.5, **kw)
    out = tr.step(batch(3))
    assert eng.calls == [("zero_grad", (3, T)), ("forward", 3), ("loss", 3, 3), ("loss_backward", 3.0, 0.5 / (T + 2 - 1)), ("backward", "dl"),
                         ("adamw_step", 3.0)]
    assert sorted(out) == ["kl", "lm_loss", "loss"] and sorted(tr.window) == ["kl", "lm_loss", "loss", "rows"]
    assert sorted(tr.evaluate_batch(batch(2))) == ["kl", "loss", "total"]
    assert tr.ul_weight == 0.0


def test_with_a_weight_the_trainer_makes_the_new_calls():
    w = 0.5
    tr, eng = make(lr=1e-3, ul_weight=w)
    assert eng.calls == [("set_ul_exclude", (0, 1, 2, 100, 102))]              # uploaded once, at construction
    eng.calls.clear()
    out = tr.step(batch(3))
    ntok, n, gscale = T - 1, 3, 3.0
    assert eng.calls == [("zero_grad", (3, T)), ("forward", 3), ("loss", 3, 3), ("ul_loss", 3),
                         ("loss_backward_ul", gscale, 0.0, w / (ntok * n) * gscale), ("backward", "dl_ul"), ("adamw_step", 3.0)]
    assert eng.calls[4][3] == pytest.approx(w / ntok, rel=1e-15)
    assert sorted(out) == ["kl", "lm_loss", "loss", "ul"] and float(out["ul"]) == 0.75
    assert sorted(tr.window) == ["kl", "lm_loss", "loss", "rows", "ul"] and float(tr.window["ul"]) == 0.75
    ev = tr.evaluate_batch(batch(2))
    assert sorted(ev) == ["kl", "loss", "total", "ul"] and float(ev["ul"]) == 3.0
    assert float(ev["total"]) == 1.0 + tr.alpha * 1.0                          # the reference's validation loss: no term in it
    assert "set_ul_exclude" not in eng.names()


def test_a_window_weights_the_term_by_rows():
    tr, eng = make(lr=1e-3, ul_weight=0.5, ul_exclude_ids=[7], accumulation_steps=2)
    assert eng.calls == [("set_ul_exclude", (7,))]
    o1 = tr.step(batch(3))
    o2 = tr.step(batch(1))
    assert float(o1["ul"]) == 0.75 and float(o2["ul"]) == 0.25
    assert float(tr.window["ul"]) == pytest.approx((3 * 0.75 + 1 * 0.25) / 4, rel=1e-6) and tr.window["rows"] == 4
    assert float(tr.window["loss"]) == pytest.approx(1.0) and float(tr.window["kl"]) == pytest.approx((3 * 1.5 + 0.5) / 4)
    assert [c[3] for c in eng.calls if c[0] == "loss_backward_ul"] == [0.5 / (6 * 3) * 3.0, 0.5 / (6 * 1) * 1.0]


@pytest.mark.parametrize("bad", [-0.1, NAN, INF, "x", None, True, [0.5]])
def test_the_weight_is_validated(bad):
    with pytest.raises(ValueError, match="ul_weight"):
        make(ul_weight=bad)


@pytest.mark.parametrize("bad", [list(range(33)), (1, -2), (1, 2.0), ("a",), 5, (True,)])
def test_the_exclude_ids_are_validated(bad):
    with pytest.raises(ValueError, match="ul_exclude_ids"):
        make(ul_weight=0.5, ul_exclude_ids=bad)


def test_hparams_round_trip():
    tr, eng = make(lr=1e-3, ul_weight=0.5, ul_exclude_ids=[7, 8])
    sd = tr.state_dict()
    assert sd["hparams"]["ul_weight"] == 0.5 and sd["hparams"]["ul_exclude_ids"] == (7, 8)
    assert make(PlainEngine, lr=1e-3)[0].state_dict()["hparams"]["ul_weight"] == 0.0
    assert make(PlainEngine, lr=1e-3)[0].state_dict()["hparams"]["ul_exclude_ids"] == (0, 1, 2, 100, 102)
    other, oeng = make(lr=1e-3, ul_weight=0.25)
    other.load_state_dict(sd)
    assert other.ul_weight == 0.25 and other.ul_exclude_ids == (0, 1, 2, 100, 102)        # the trainer's own, like lr
    assert oeng.names().count("set_ul_exclude") == 1
    plain, _ = make(PlainEngine, lr=1e-3)
    plain.load_state_dict(sd)                                                               # ... and a trainer without the term stays without
    assert plain.ul_weight == 0.0
    old = dict(sd, hparams={k: v for k, v in sd["hparams"].items() if not k.startswith("ul_")})
    other.load_state_dict(old)                                                              # a checkpoint from before the term
    assert other.ul_weight == 0.25


# ---- 4: the yardstick
def _worst(got, ref, allow):
    return float(((got.double() - ref).abs() / allow).max())


@pytest.mark.parametrize("geo", sorted(set((g[0], g[3]) for g in R.geometries())), ids=lambda g: "V%d-L%d" % g)
def test_float32_restatement_stays_inside_the_bounds(geo):
    """Every case of tests/test_ul_ops_gpu.py (both storage types of the logits, both P, with and without the exclude list, both
    (lm_coef, gscale) pairs, u = 0 and U) through a float32 evaluation of the kernels' expressions: forward quantities, d(logits) as fp32,
    as bf16 and as a (hi | lo) pair, every element.  A bound this cannot meet is a wrong derivation, not a kernel bug."""
    V, L = geo
    worst = {}
    for P in R.PS:
        for bf in (False, True):
            x, topic, tg, lse, coef, pl = R.case(V, P, L, bf)
            for with_list in (True, False):
                ex = R.DEFAULT_EXCLUDE if with_list else None
                fw = R.reference(V, P, L, bf, with_list)
                f32 = R.forward32(x, lse, tg, P, V, ex, float(R.B))
                assert torch.equal(f32["mask"], fw["mask"])
                for q, al in (("ul_row", "allow_row"), ("S", "allow_S"), ("ul_sample", "allow_sample"), ("ul", "allow_ul")):
                    worst[q] = max(worst.get(q, 0.0), _worst(f32[q], fw[q], fw[al]))
                cm, cc = pl["clamped"]
                assert bool(fw["clamped"][cm, cc]) and float(f32["g"][cm, cc]) == 0.0
                S32 = fw["S"].float()
                for lm_coef, gscale in R.COMBOS:
                    for u in (0.0, R.U):
                        d, allow, rc = R.backward(fw, S32, topic, tg, coef, gscale, lm_coef, u, P, V)
                        d32 = R.backward32(f32, S32, topic, tg, coef, gscale, lm_coef, u, P, V)
                        worst["d f32"] = max(worst.get("d f32", 0.0), _worst(d32, d, R.out_allow(d, allow, "f32") + 1e-300))
                        hi = d32.bfloat16()
                        worst["d bf16"] = max(worst.get("d bf16", 0.0), _worst(hi, d, R.out_allow(d, allow, "bf16") + 1e-300))
                        lo = (d32 - hi.float()).bfloat16()
                        worst["d hi+lo"] = max(worst.get("d hi+lo", 0.0), _worst(hi.double() + lo.double(), d, R.out_allow(d, allow, "x3") + 1e-300))
    print("V=%d L=%d: worst error / allowed of the float32 restatement: %s" % (V, L, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst
