"""Optimizer parameter groups, host side (mmtg_amd/param_groups.py, mmtg_param_groups_check, the trainer's record): no GPU.

The builder turns torch-style specs with fnmatch patterns into the (begin, end, group) table the grouped step kernels walk;
tests/test_param_groups_gpu.py holds the kernels and the trainer to it."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.configs import gpt2_config, make_model_cfgs
from mmtg_amd.engine import ParamLayout
from mmtg_amd.param_groups import build_param_groups
from mmtg_amd.trainer import MMTGTrainer

NO_DECAY = [{"params": ["*bias*", "*ln_*"], "weight_decay": 0.0}]


@pytest.fixture(scope="module")
def layout():
    return ParamLayout(make_model_cfgs(seq_len=5), gpt2_config(n_layer=2, vocab_size=160, n_positions=256))


def _covered(plan):
    """element -> group over the whole flat buffer (-1: in no segment)"""
    m = np.full(plan.total, -1, dtype=np.int64)
    for b, e, g in plan.segments:
        assert (m[b:e] == -1).all()
        m[b:e] = g
    return m


def test_first_match_wins_and_the_implicit_group_is_last(layout):
    specs = [{"params": "*ln_1*", "lr_scale": 0.5}, {"params": ["*bias*", "*ln_*"], "weight_decay": 0.0}, {"params": "encoder.*", "frozen": True}]
    plan = build_param_groups(layout, specs, 0.1)
    assert len(plan.groups) == 4 and plan.groups[-1]["spec"] is None
    assert [g["lr_scale"] for g in plan.groups] == [0.5, 1.0, 1.0, 1.0]
    assert [g["weight_decay"] for g in plan.groups] == [0.1, 0.0, 0.1, 0.1]          # None = the trainer's value
    assert [g["frozen"] for g in plan.groups] == [False, False, True, False]
    k = "decoder.gpt2.transformer.h.0.ln_1.bias"              # matches specs 0 and 1: the first wins
    assert plan.group_of(k) == 0
    assert plan.group_of("decoder.gpt2.transformer.h.0.ln_2.bias") == 1
    assert plan.group_of("encoder.topic_fc.bias") == 1        # a bias before it is an encoder tensor
    assert plan.group_of("encoder.topic_fc.weight") == 2
    assert plan.group_of("decoder.gpt2.transformer.wte.weight") == 3
    # every key is in exactly one group, and the table says the same as the key lists
    assert sorted(k for g in plan.groups for k in g["keys"]) == sorted(layout.keys)
    cover = _covered(plan)
    for i, g in enumerate(plan.groups):
        assert g["parameters"] == sum(layout.entries[k][2] for k in g["keys"]) == int((cover == i).sum())
        for k in g["keys"]:
            off, _, n = layout.entries[k]
            assert (cover[off:off + n] == i).all(), k
    assert plan.specs == specs and plan.specs is not specs
    hip.param_groups_check(plan.segments, len(plan.groups), plan.total)


def test_segments_are_exact_key_ranges_merged_where_they_touch(layout):
    plan = build_param_groups(layout, NO_DECAY, 0.1)
    segs = plan.segments
    assert segs.dtype == np.int64 and segs.shape[1] == 3
    assert (segs[:, 0] < segs[:, 1]).all() and (segs[1:, 0] >= segs[:-1, 1]).all()          # non-empty, sorted, disjoint
    # no segment contains a pad element: the covered elements are exactly the keys' elements (gaps between packs and wte's tail
    # pad are in no entry)
    in_key = np.zeros(layout.total, dtype=bool)
    for off, _, n in layout.entries.values():
        in_key[off:off + n] = True
    assert not in_key.all()                                   # this layout has pads (wte: 160 rows of a 256-row pack)
    assert ((_covered(plan) >= 0) == in_key).all()
    woff, _, wn = layout.entries["decoder.gpt2.transformer.wte.weight"]
    assert [woff, woff + wn, 1] in segs.tolist() and layout.pack_range["wte"][1] > wn
    # neighbours of one group are one segment where they touch (the three query / key / value matrices of a pack) ...
    q = layout.entries["text_inner_atten_layer.query.weight"]
    v = layout.entries["text_inner_atten_layer.value.weight"]
    assert [q[0], v[0] + v[2], 1] in segs.tolist()
    # ... and only there: two neighbours of one group never touch
    same = segs[1:, 2] == segs[:-1, 2]
    assert (segs[1:, 0][same] > segs[:-1, 1][same]).all()
    # the one-element att_matrices.*.bias keys: boundaries inside a 16-byte vector
    b = [layout.entries["mm_atten_layer.att_matrices.%d.bias" % i][0] for i in range(5)]
    assert sum(1 for o in b if o % 4) == 3
    assert [b[0], b[0] + 5, 0] in segs.tolist() and (b[0] + 5) % 4 == 1
    one = build_param_groups(layout, [{"params": "mm_atten_layer.att_matrices.2.bias", "lr_scale": 2.0}], 0.0)
    rows = one.segments.tolist()
    i = rows.index([b[2], b[2] + 1, 0])
    assert b[2] % 4 == 2 and rows[i - 1][1:] == [b[2], 1] and rows[i + 1] == [b[2] + 1, b[2] + 3, 1]


def test_full_configuration_no_decay_split():
    lay = ParamLayout(make_model_cfgs(), gpt2_config())
    plan = build_param_groups(lay, NO_DECAY, 0.1)
    assert len(lay.keys) == 192 and len(plan.segments) == 116
    assert len(plan.groups[0]["keys"]) + len(plan.groups[1]["keys"]) == 192
    assert sum(1 for i in range(5) if lay.entries["mm_atten_layer.att_matrices.%d.bias" % i][0] % 4) == 3
    hip.param_groups_check(plan.segments, 2, lay.total)


def test_empty_groups_and_a_catch_all_are_allowed(layout):
    plan = build_param_groups(layout, [{"params": "*"}, {"params": "encoder.*", "frozen": True}], 0.0)
    assert [len(g["keys"]) for g in plan.groups] == [len(layout.keys), 0, 0]
    assert set(plan.segments[:, 2].tolist()) == {0}
    plan = build_param_groups(layout, [], 0.25)
    assert len(plan.groups) == 1 and plan.groups[0]["weight_decay"] == 0.25 and len(plan.groups[0]["keys"]) == len(layout.keys)
    assert len(build_param_groups(layout, [{"params": []}], 0.0).groups[0]["keys"]) == 0


def test_builder_errors_name_the_offender(layout):
    with pytest.raises(ValueError, match=r"'\*biass\*' matches no parameter"):
        build_param_groups(layout, [{"params": ["*ln_*", "*biass*"]}], 0.0)
    with pytest.raises(ValueError, match="17 groups"):
        build_param_groups(layout, [{"params": "*"}] * 16, 0.0)
    assert len(build_param_groups(layout, [{"params": "*"}] * 15, 0.0).groups) == 16
    for bad in (-0.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match=r"param_groups\[1\]: lr_scale"):
            build_param_groups(layout, [{"params": "*bias*"}, {"params": "*", "lr_scale": bad}], 0.0)
    for bad in (-0.01, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match=r"param_groups\[0\]: weight_decay"):
            build_param_groups(layout, [{"params": "*", "weight_decay": bad}], 0.0)
    with pytest.raises(ValueError, match="weight_decay"):
        build_param_groups(layout, [{"params": "*"}], -1.0)
    with pytest.raises(ValueError, match=r"param_groups\[0\]: unknown key 'lr'"):
        build_param_groups(layout, [{"params": "*", "lr": 1e-3}], 0.0)
    with pytest.raises(ValueError, match="no 'params'"):
        build_param_groups(layout, [{"lr_scale": 1.0}], 0.0)
    with pytest.raises(ValueError, match="frozen"):
        build_param_groups(layout, [{"params": "*", "frozen": 1}], 0.0)


def _check(rows, ngroups, n):
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    L = hip.lib()
    rc = L.mmtg_param_groups_check(a.ctypes.data if len(a) else None, len(a), ngroups, n)
    return rc, L.mmtg_last_error().decode()


def test_param_groups_check_on_the_host():
    """good tables pass; each bad one is refused with its message.  The entry is host arithmetic: this test runs without a GPU."""
    good = [(0, 1, 0), (1, 2, 1), (2, 5, 2), (8, 100, 1)]
    assert _check(good, 3, 100)[0] == 0
    assert _check([], 1, 100)[0] == 0                          # nsegs = 0
    assert _check(good, 16, 100)[0] == 0                       # groups without segments
    assert _check([(i, i + 1, i % 16) for i in range(1024)], 16, 1024)[0] == 0
    bad = {
        "not sorted": ([(8, 16, 0), (0, 4, 0)], 1, 100),
        "overlaps": ([(0, 8, 0), (4, 12, 0)], 1, 100),
        "is empty": ([(0, 4, 0), (6, 6, 0)], 1, 100),
        "is outside": ([(0, 4, 0), (96, 101, 0)], 1, 100),
        "has group 2": ([(0, 4, 0), (4, 8, 2)], 2, 100),
        "has group -1": ([(0, 4, -1)], 2, 100),
        "ngroups = 17": ([(0, 4, 0)], 17, 100),
        "ngroups = 0": ([(0, 4, 0)], 0, 100),
        "nsegs = 1025": ([(i, i + 1, 0) for i in range(1025)], 1, 2000),
    }
    for msg, (rows, ng, n) in bad.items():
        rc, err = _check(rows, ng, n)
        assert rc != 0 and "param_groups_check: " in err and msg in err, (msg, rc, err)
    rc, err = _check([(-4, 4, 0)], 1, 100)
    assert rc != 0 and "is outside" in err
    with pytest.raises(RuntimeError, match="overlaps segment 0"):
        hip.param_groups_check([(0, 8, 0), (4, 12, 0)], 1, 100)


def test_launch_entries_check_the_table_before_any_device_call():
    """sumsq_groups and adamw_groups run the same checks on the host copy first (fake device pointers, no GPU touched), and
    adamw_groups refuses a bad group record"""
    L = hip.lib()
    p = [0x7000000000 + (i << 24) for i in range(8)]
    bad = np.asarray([(0, 8, 0), (4, 12, 0)], dtype=np.int64)
    assert L.mmtg_sumsq_groups(p[0], 100, p[1], bad.ctypes.data, 2, 1, 0, p[2], p[3], 1 << 20, None) != 0
    assert b"sumsq_groups: segment 1" in L.mmtg_last_error() and b"overlaps" in L.mmtg_last_error()
    rec = (hip.ParamGroup * 1)(hip.ParamGroup(1.0, 0.0, 0, 0))
    assert L.mmtg_adamw_groups(p[0], p[1], p[2], p[3], None, None, 100, p[4], bad.ctypes.data, 2, ctypes.addressof(rec), 1,
                               1e-3, 0.9, 0.999, 1e-6, 1, None, 1.0, 1.0, None, None) != 0
    assert b"adamw_groups: segment 1" in L.mmtg_last_error()
    good = np.asarray([(0, 8, 0)], dtype=np.int64)
    for field, value in (("lr_scale", -1.0), ("lr_scale", float("nan")), ("weight_decay", float("inf")), ("weight_decay", -0.1)):
        rec = (hip.ParamGroup * 1)(hip.ParamGroup(1.0, 0.0, 0, 0))
        setattr(rec[0], field, value)
        assert L.mmtg_adamw_groups(p[0], p[1], p[2], p[3], None, None, 100, p[4], good.ctypes.data, 1, ctypes.addressof(rec), 1,
                                   1e-3, 0.9, 0.999, 1e-6, 1, None, 1.0, 1.0, None, None) != 0
        assert b"adamw_groups: group 0 has " + field.encode() in L.mmtg_last_error()
    assert L.mmtg_sumsq_groups_ws(2098179, 4) == 4 * 2048 and L.mmtg_sumsq_groups_ws(5, 16) == 16


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmtg_hip.h")).read()
    lib = ctypes.CDLL(hip.lib_path())
    for name in ("mmtg_param_groups_check", "mmtg_sumsq_groups_ws", "mmtg_sumsq_groups", "mmtg_adamw_groups"):
        assert name + "(" in header and name in hip.exported_symbols() and name in hip._SIGS and hasattr(lib, name)
    assert len(hip._SIGS["mmtg_sumsq_groups"][0]) == 11 and len(hip._SIGS["mmtg_adamw_groups"][0]) == 22
    assert ctypes.sizeof(hip.ParamGroup) == 16
    assert hip.lib().mmtg_abi_version() == hip.ABI_VERSION == 12
    assert callable(hip.sumsq_groups) and callable(hip.adamw_groups)


def test_trainer_records_the_specs(layout):
    """The trainer's host side around a stand-in for the model (a real engine needs the GPU): the plan is built from the engine's
    layout with the trainer's weight_decay, state_dict()['hparams'] records the specs, load_state_dict keeps the trainer's own."""
    def stand_in():
        eng = types.SimpleNamespace(layout=layout, dev=torch.device("cpu"), opt_m=None, opt_v=None, step_count=0, drop_seed=5)
        return types.SimpleNamespace(engine=lambda: eng)

    specs = [{"params": "decoder.gpt2.*", "frozen": True}, {"params": ["*bias*"], "weight_decay": 0.0, "lr_scale": 0.5}]
    tr = MMTGTrainer(stand_in(), lr=1e-3, weight_decay=0.1, param_groups=specs)
    sd = tr.state_dict()
    assert sd["hparams"]["param_groups"] == specs and sd["hparams"]["param_groups"] is not specs
    assert tr.current_lr() == 1e-3                             # the base rate: groups scale it
    d = tr.describe_groups()
    assert [g["spec"] for g in d] == specs + [None]
    assert [g["frozen"] for g in d] == [True, False, False] and [g["weight_decay"] for g in d] == [0.1, 0.0, 0.1]
    assert sum(g["tensors"] for g in d) == len(layout.keys)
    assert sum(g["parameters"] for g in d) == sum(e[2] for e in layout.entries.values())
    assert d[0]["tensors"] == sum(1 for k in layout.keys if k.startswith("decoder.gpt2."))
    assert tr.groups.frozen_mask == 1 and tr.groups.ngroups == 3 and tr.groups.nsegs == len(tr.group_plan.segments)
    plain = MMTGTrainer(stand_in(), lr=1e-3)
    assert plain.state_dict()["hparams"]["param_groups"] is None and plain.describe_groups() == [] and plain.groups is None
    other = MMTGTrainer(stand_in(), lr=1e-3, param_groups=[{"params": "*", "lr_scale": 2.0}])
    other.load_state_dict(sd)
    assert other.state_dict()["hparams"]["param_groups"] == [{"params": "*", "lr_scale": 2.0}] and other.eng.drop_seed == 5
    with pytest.raises(ValueError, match="matches no parameter"):
        MMTGTrainer(stand_in(), param_groups=[{"params": "decoder.gpt3.*"}])
