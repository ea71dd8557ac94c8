"""Optimizer parameter groups on the GPU: mmtg_sumsq_groups and mmtg_adamw_groups at their vector, workgroup, partial and grid
edges, and the trainer with frozen tensors, a per-group learning rate and the no_decay split.

The grouped kernels tile like the plain ones (one 16-byte vector per lane and pass, 1024 elements per workgroup and pass, at most
2048 workgroups), so EDGE crosses the plain kernels' edges: the vector boundary at 4, a workgroup chunk at 1024, the 256-partial
edge at 262144, the end of the first grid trip at 2097152, and a last segment that ends at n in the scalar tail; [6, 8) and
[2098176, 2098177) belong to no segment.  The reference of the update is the existing mmtg_adamw, run per group on copies of the
same buffers with that group's (lr, wd): the grouped result must equal it bit for bit on the group's elements, and elements of
frozen groups and gaps (NaN gradients, sentinel planes) must keep every bit."""
import math

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.param_groups import ParamGroupPlan

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
BF = torch.bfloat16
SENT = 1234.0

GROUPS = [dict(lr_scale=1.0, weight_decay=0.01, frozen=False), dict(lr_scale=0.1, weight_decay=0.0, frozen=False),
          dict(lr_scale=3.0, weight_decay=0.1, frozen=False), dict(lr_scale=1.0, weight_decay=0.0, frozen=True)]
EDGE_N = 2098179            # one element past a scalar tail behind the plain kernel's last full grid (2048 workgroups x 1024)
EDGE = [(0, 1, 0), (1, 2, 1), (2, 5, 2), (5, 6, 3), (8, 1023, 1), (1023, 1025, 0), (1025, 262143, 2), (262143, 262149, 3),
        (262149, 2097150, 0), (2097150, 2097153, 1), (2097153, 2098176, 2), (2098177, 2098179, 1)]
TABLES = {
    1: [(0, 1, 2)],
    5: [(0, 1, 0), (1, 2, 3), (3, 5, 2)],                                           # 1 frozen, 2 a gap, ends at n
    1027: [(0, 3, 1), (3, 4, 3), (4, 8, 0), (9, 1024, 2), (1024, 1027, 1)],          # 8 a gap; a second workgroup's scalar tail
    EDGE_N: EDGE,
}
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, max_norm=1.0)
STEPS = [1, 2, 1000]
# sqrt(3e4) = 173: clipped with and without the count (173 / 7 = 25 > max_norm); sqrt(1e-4) = 0.01: never
NORMSQ = {"active": 3.0e4, "inactive": 1.0e-4}
CFGS = [(ns, cnt) for ns in ("active", "inactive") for cnt in (None, 7.0)]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _table(n):
    plan = ParamGroupPlan(np.asarray(TABLES[n], dtype=np.int64), GROUPS, None, n)
    return hip.GroupTable(plan, DEV)


def _group_map(n):
    """element -> group (-1: a gap) on the CPU"""
    m = torch.full((n,), -1, dtype=torch.int64)
    for b, e, g in TABLES[n]:
        m[b:e] = g
    return m


def _live(n):
    gm = _group_map(n)
    return (gm >= 0) & (gm != 3)


def group_lr(lr, scale):
    """the fp32 rounding of (double)lr * (double)lr_scale, from the fp32 values the entry receives"""
    return float(np.float32(np.float64(np.float32(lr)) * np.float64(np.float32(scale))))


# =====================================================================================================================
# sumsq_groups
# =====================================================================================================================
@pytest.mark.parametrize("n", sorted(TABLES))
def test_sumsq_groups_exact(n):
    """integers in -2 .. 2: every partial sum is an integer below 4 n < 2^24, exact in fp32 in any order.  Frozen and gap
    elements are NaN: any read of them shows up in a sum."""
    assert 4 * n < 2 ** 24
    tab = _table(n)
    gm = _group_map(n)
    x = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(n))
    ref = [int((x[gm == g] ** 2).sum()) if g != 3 else 0 for g in range(4)]
    xf = x.float()
    xf[~_live(n)] = NAN
    xd = xf.to(DEV)
    need = int(hip.lib().mmtg_sumsq_groups_ws(n, 4))
    assert need == 4 * min(2048, (n // 4 + 1 + 255) // 256)
    ws = torch.full((need,), NAN, device=DEV)
    out = torch.full((7,), SENT, device=DEV)                # a sentinel on either side of the five outputs

    def call(ws_floats):
        hip._check(hip.lib().mmtg_sumsq_groups(xd.data_ptr(), n, hip._p(tab.segs_dev), tab.segs_host.ctypes.data, tab.nsegs, 4,
                                               tab.frozen_mask, out[1:].data_ptr(), ws.data_ptr(), ws_floats,
                                               torch.cuda.current_stream().cuda_stream), "sumsq_groups")

    call(need)
    first = out.cpu()
    assert first[1:5].tolist() == [float(r) for r in ref], (first.tolist(), ref)
    assert first[5].item() == float(sum(ref))
    assert first[0].item() == SENT and first[6].item() == SENT
    assert bool(torch.isfinite(ws).all())
    out[1:6] = 1.0e6                                         # written, not accumulated
    call(need)
    assert torch.equal(_bits(out.cpu()), _bits(first))
    with pytest.raises(RuntimeError, match="workspace"):     # one float short
        call(need - 1)
    assert torch.equal(_bits(out.cpu()), _bits(first))


def test_sumsq_groups_through_the_binding_with_an_empty_table():
    """hip.sumsq_groups; a table without segments writes zeros and reads nothing"""
    n = 1027
    tab = hip.GroupTable(ParamGroupPlan(np.zeros((0, 3), dtype=np.int64), GROUPS[:2], None, n), DEV)
    out = torch.full((3,), SENT, device=DEV)
    hip.sumsq_groups(torch.full((n,), NAN, device=DEV), n, tab, out)
    assert out.tolist() == [0.0, 0.0, 0.0]
    tab = _table(n)
    x = torch.ones(n)
    x[~_live(n)] = NAN
    out = torch.full((5,), SENT, device=DEV)
    hip.sumsq_groups(x.to(DEV), n, tab, out)
    assert out.tolist() == [4.0, 6.0, 1015.0, 0.0, 1025.0]


# =====================================================================================================================
# adamw_groups
# =====================================================================================================================
def _adam_data(n, seed, steps):
    """p, and per step a gradient: |g| log-uniform in [1e-6, 10], exact zeros at every 7th element (index 3, 10, ...: with m = v = 0
    the update there must be exactly 0), and one sign per element over the steps, so that no element of m is a cancelling sum
    and "2^-20 relative" is meaningful for it (the data of tests/test_train_ops_gpu.py, restated)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    gs = []
    for _ in range(steps):
        mag = torch.exp(torch.rand(n, generator=g).double() * math.log(1e7) + math.log(1e-6)).float().clamp(1e-6, 10.0)
        gr = sign * mag
        gr[3::7] = 0.0
        gs.append(gr)
    return p, gs


_DATA = {}


def _data(n):
    """one data set per n, shared by every case and left unchanged: p and three gradients on the device, NaN gradients at the
    frozen and gap elements"""
    if n not in _DATA:
        p, gs = _adam_data(n, 7 * n + 1, 3)
        dead = ~_live(n)
        for g in gs:
            g[dead] = NAN
        _DATA[n] = (p.to(DEV), [g.to(DEV) for g in gs], _group_map(n).to(DEV))
    return _DATA[n]


def _buffers(n, p, planes, offset):
    """p, m, v, p_bf16, p_lo on the device.  offset "p": the parameters start one float past a 16-byte boundary, "pc": the bf16
    copy one bf16 past an 8-byte boundary (either sends every vector down the element path).  The planes start as sentinels."""
    po = 1 if offset == "p" else 0
    dp = torch.zeros(n + 8, device=DEV)[po:po + n]
    dp.copy_(p)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    co = 1 if offset == "pc" else 0
    pc = torch.full((n + 8,), SENT, device=DEV, dtype=BF)[co:co + n] if planes >= 1 else None
    pl = torch.full((n + 8,), SENT, device=DEV, dtype=BF)[:n] if planes >= 2 else None
    assert dp.data_ptr() % 16 == 4 * po and (pc is None or pc.data_ptr() % 8 == 2 * co)
    return [dp, m, v, pc, pl]


def _clone(bufs):
    return [None if b is None else b.clone() for b in bufs]


def _grouped_step(n, tab, bufs, g, step, ns, cnt):
    hip.adamw_groups(bufs[0], g, bufs[1], bufs[2], bufs[3], n, tab, HP["lr"], HP["b1"], HP["b2"], HP["eps"], step, ns, HP["max_norm"],
                     grad_scale=1.0, count=cnt, p_lo=bufs[4])


def _plain_step(n, bufs, g, step, ns, cnt, lr, wd):
    hip.adamw(bufs[0], g, bufs[1], bufs[2], bufs[3], n, lr, HP["b1"], HP["b2"], HP["eps"], wd, step, ns, HP["max_norm"],
              grad_scale=1.0, count=cnt, p_lo=bufs[4])


NAMES = ("p", "m", "v", "p_bf16", "p_lo")


def _run_against_the_plain_kernel(n, cfg, planes, offset):
    ns_name, cnt = cfg
    tab = _table(n)
    p, grads, gm = _data(n)
    ns = torch.tensor([NORMSQ[ns_name]], device=DEV)
    cd = None if cnt is None else torch.tensor([cnt], device=DEV)
    bufs = _buffers(n, p, planes, offset)
    dead = (gm < 0) | (gm == 3)
    start = _clone(bufs)
    name = "n=%d normsq=%s count=%s planes=%d offset=%s" % (n, ns_name, cnt, planes, offset)
    for step, g in zip(STEPS, grads):
        before = _clone(bufs)                    # (aligned copies: the plain kernel's two paths are bit-equal, test_train_ops_gpu.py)
        _grouped_step(n, tab, bufs, g, step, ns, cd)
        for k in sorted({grp for _, _, grp in TABLES[n]} - {3}):         # (the small tables do not hold every group)
            ref = _clone(before)
            _plain_step(n, ref, g, step, ns, cd, group_lr(HP["lr"], GROUPS[k]["lr_scale"]), GROUPS[k]["weight_decay"])
            sel = gm == k
            for what, a, b in zip(NAMES, bufs, ref):
                if a is not None:
                    assert torch.equal(_bits(a)[sel], _bits(b)[sel]), "%s step %d group %d: %s differs from mmtg_adamw" % (name, step, k, what)
            # (the group's elements really moved, and the planes are the planes of p)
            assert not torch.equal(_bits(bufs[0])[sel], _bits(before[0])[sel]) or n < 8
        if bufs[3] is not None:
            live = ~dead
            assert torch.equal(_bits(bufs[3])[live], _bits(bufs[0].bfloat16())[live])
    for what, a, b in zip(NAMES, bufs, start):
        if a is not None:
            assert torch.equal(_bits(a)[dead], _bits(b)[dead]), "%s: %s of a frozen or gap element changed" % (name, what)
    assert bool(torch.isfinite(bufs[0]).all()) and bool(torch.isfinite(bufs[1]).all()) and bool(torch.isfinite(bufs[2]).all())


@pytest.mark.parametrize("n", sorted(TABLES))
def test_adamw_groups_equals_the_plain_kernel_per_group(n):
    """three state-carrying steps; clip active and inactive, with and without the row count, planes 0 / 1 / 2, aligned pointers and
    the two misaligned variants"""
    for i, cfg in enumerate(CFGS):
        planes = i % 3
        _run_against_the_plain_kernel(n, cfg, planes, None)
        _run_against_the_plain_kernel(n, cfg, planes, "p")
        _run_against_the_plain_kernel(n, cfg, max(planes, 1), "pc")
    _run_against_the_plain_kernel(n, CFGS[1], 2, None)         # (i % 3 reaches the lo plane with one configuration only)


@pytest.mark.parametrize("count", [0.0, -1.0, NAN])
@pytest.mark.parametrize("n", [5, 1027])
def test_adamw_groups_skips_the_step_without_rows(n, count):
    """*count not greater than 0 (an empty global batch; NaN included): every buffer keeps its bits"""
    p, grads, _ = _data(n)
    g = torch.Generator().manual_seed(n)
    bufs = [p.clone(), torch.randn(n, generator=g).to(DEV), torch.rand(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV).to(BF),
            torch.randn(n, generator=g).to(DEV).to(BF)]
    keep = _clone(bufs)
    _grouped_step(n, _table(n), bufs, grads[0], 1, torch.tensor([3.0e4], device=DEV), torch.tensor([count], device=DEV))
    for b, k in zip(bufs, keep):
        assert torch.equal(_bits(b), _bits(k))


def test_adamw_groups_rejects_a_lo_plane_without_the_hi_plane():
    n = 1027
    z = [torch.zeros(n, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError, match="lo plane"):
        hip.adamw_groups(z[0], z[1], z[2], z[3], None, n, _table(n), 1e-3, 0.9, 0.999, 1e-6, 1, None, 1.0, p_lo=torch.zeros(n, device=DEV, dtype=BF))


def _adam_formula64(p, g, m, v, lr, wd, normsq, count, step):
    """the header's formula in float64 on the fp32 values the kernel receives; returns p, m, v and the update"""
    h = {k: np.float32(x) for k, x in HP.items()}
    gsc = np.float64(1.0)
    if count is not None:
        gsc = gsc * (1.0 / np.float64(np.float32(count)))
    coef = gsc
    if normsq is not None:
        nrm = np.sqrt(np.float64(np.float32(normsq))) * gsc
        coef = coef * min(1.0, np.float64(h["max_norm"]) / (nrm + np.float64(np.float32(1e-6))))
    b1, b2 = float(h["b1"]), float(h["b2"])
    lr = np.float64(np.float32(lr))
    ss = lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
    gi = g.astype(np.float64) * coef
    mi = b1 * m.astype(np.float64) + (1.0 - b1) * gi
    vi = b2 * v.astype(np.float64) + (1.0 - b2) * gi * gi
    upd = ss * (mi / (np.sqrt(vi) + np.float64(h["eps"])))
    pi = p.astype(np.float64) - upd
    if wd > 0:
        pi = pi - lr * np.float64(np.float32(wd)) * pi
    return pi, mi, vi, upd


def test_adamw_groups_against_float64():
    """Independent of mmtg_adamw: n = 1027, clip active, count 7, three steps, each judged alone against the float64 formula with the
    group's (lr, wd), on the fp32 state the step started from.  The bounds are those tests/test_train_ops_gpu.py derives for the
    plain kernel (the arithmetic is the same): m and v within 2^-20 relative; p within 2^-23 |p| + 2^-20 |update|."""
    n, cnt = 1027, 7.0
    tab = _table(n)
    p, grads, gm = _data(n)
    gm = gm.cpu().numpy()
    ns = torch.tensor([NORMSQ["active"]], device=DEV)
    bufs = _buffers(n, p, 0, None)
    for step, g in zip(STEPS, grads):
        p0, m0, v0 = (b.cpu().numpy() for b in bufs[:3])
        _grouped_step(n, tab, bufs, g, step, ns, torch.tensor([cnt], device=DEV))
        p1, m1, v1 = (b.cpu().numpy().astype(np.float64) for b in bufs[:3])
        gh = g.cpu().numpy()
        for k in range(3):
            sel = gm == k
            pr, mr, vr, upd = _adam_formula64(p0[sel], gh[sel], m0[sel], v0[sel], group_lr(HP["lr"], GROUPS[k]["lr_scale"]),
                                              GROUPS[k]["weight_decay"], NORMSQ["active"], cnt, step)
            assert (np.abs(m1[sel] - mr) <= np.abs(mr) * 2.0 ** -20).all(), (step, k, "m")
            assert (np.abs(v1[sel] - vr) <= np.abs(vr) * 2.0 ** -20).all(), (step, k, "v")
            assert (np.abs(p1[sel] - pr) <= np.abs(pr) * 2.0 ** -23 + np.abs(upd) * 2.0 ** -20).all(), (step, k, "p")
            assert np.abs(upd).max() > 0


# =====================================================================================================================
# trainer: the two-layer, V = 160, 12-row model of tests/test_wgrad_ring_gpu.py, bf16, dropout 0.1 with a fixed drop_seed
# =====================================================================================================================
NO_DECAY = [{"params": ["*bias*", "*ln_*"], "weight_decay": 0.0}]
BIG = 1e9                   # max_norm that never clips: the clip coefficient is exactly 1, the norm's summation order cannot show


def _setup():
    from mmtg_amd import synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    S, V = 5, 160
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    gcfg = gpt2_config(n_layer=2, vocab_size=V, n_positions=256, embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1)
    weights = synth.make_weights(mcfg, gcfg, seed=100)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in synth.make_batch(12, mcfg, dcfg, V, seed=7).items()}
    return mcfg, dcfg, gcfg, V, weights, batch, synth.make_token_table(V, seed=101)


_SETUP = []


def _trainer(state=None, mode="bf16", **kw):
    from mmtg_amd import MMTG
    from mmtg_amd.trainer import MMTGTrainer
    if not _SETUP:
        _SETUP.append(_setup())
    mcfg, dcfg, gcfg, V, weights, batch, table = _SETUP[0]
    model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, token_table=table, compute_dtype=mode)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()} if state is None else state)
    model.to(DEV).train()
    kw.setdefault("lr", 1e-3)
    tr = MMTGTrainer(model, alpha=0.2, **kw)
    tr.eng.drop_seed = 4242
    return tr, batch


def _state(tr):
    e = tr.eng
    return {"master": e.master.detach().clone(), "m": e.opt_m.clone(), "v": e.opt_v.clone(), "bf16": e.wc.clone()}


def _same_on(tr, a, b, keys, what):
    lay = tr.eng.layout
    for k in keys:
        off, _, n = lay.entries[k]
        for name in a:
            assert torch.equal(_bits(a[name][off:off + n]), _bits(b[name][off:off + n])), "%s: %s of %s differs" % (what, name, k)


def _adopt(tr, st):
    """continue `tr` from the parameters and moments of another run (its bf16 copies are re-derived from the masters)"""
    e = tr.eng
    e.master.copy_(st["master"])
    e.opt_m.copy_(st["m"])
    e.opt_v.copy_(st["v"])
    e.invalidate_copies()
    e.refresh_copies()


def _two_steps_against_plain_runs(grouped_kw, plains):
    """Two steps of a grouped trainer; after each, every (plain trainer kwargs, keys) pair must agree with it bit for bit on the
    keys.  The runs part ways on the OTHER keys after one step, so before the second step the plain trainers take over the
    grouped run's parameters and moments: each step is compared from one common state."""
    tr, batch = _trainer(**grouped_kw)
    others = [(_trainer(**kw)[0], keys(tr)) for kw, keys in plains]
    assert sorted(k for _, ks in others for k in ks) == sorted(tr.eng.layout.keys)
    for step in range(2):
        tr.step(batch, stage=3)
        st = _state(tr)
        for o, ks in others:
            o.step(batch, stage=3)
            assert len(ks) > 0
            _same_on(tr, st, _state(o), ks, "step %d" % (step + 1))
            _adopt(o, st)
    return tr


def test_trainer_one_catch_all_group_equals_the_plain_trainer():
    """(a) no difference without real groups: everything in one group, nothing clipped"""
    tr, batch = _trainer(max_norm=BIG, param_groups=[{"params": "*"}])
    plain, _ = _trainer(max_norm=BIG)
    for _ in range(2):
        tr.step(batch, stage=3)
        plain.step(batch, stage=3)
    a, b = _state(tr), _state(plain)
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
    assert float(a["m"].abs().max()) > 0
    assert float(tr.group_grad_norms()[1]) == 0.0                      # the implicit group is empty
    assert float(tr.group_grad_norms()[0]) == float(tr.grad_norm())


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16x3f"])
def test_trainer_groups_in_the_other_compute_modes(mode):
    """the grouped step goes through the same plane pointers as the plain call: no bf16 copy (f32), the (hi | lo) plane pair
    (bf16x3, bf16x3f).  The no_decay split with both groups at one decay and nothing clipped equals the plain trainer bit for bit,
    planes included; with the decoder frozen its planes and masters stand still."""
    tr, batch = _trainer(mode=mode, max_norm=BIG, weight_decay=0.1, param_groups=[{"params": ["*bias*", "*ln_*"]}])
    plain, _ = _trainer(mode=mode, max_norm=BIG, weight_decay=0.1)
    fr, _ = _trainer(mode=mode, param_groups=[{"params": "decoder.gpt2.*", "frozen": True}])
    fr.eng.refresh_copies()
    start = fr.eng.master.detach().clone(), None if fr.eng.wc2 is None else fr.eng.wc2.clone()
    for _ in range(2):
        tr.step(batch, stage=3)
        plain.step(batch, stage=3)
        fr.step(batch, stage=3)
    assert tr.groups.nsegs > 10
    planes = (lambda e: e.wc2) if mode != "f32" else (lambda e: None)
    assert (planes(tr.eng) is not None) == (mode != "f32")
    for a, b in ((tr.eng.master, plain.eng.master), (tr.eng.opt_m, plain.eng.opt_m), (tr.eng.opt_v, plain.eng.opt_v), (planes(tr.eng), planes(plain.eng))):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b))
    lay = fr.eng.layout
    for k in lay.keys:
        off, _, n = lay.entries[k]
        if k.startswith("decoder.gpt2."):
            assert torch.equal(_bits(fr.eng.master[off:off + n]), _bits(start[0][off:off + n])), k
            if start[1] is not None:
                assert torch.equal(_bits(fr.eng.wc2[:, off:off + n]), _bits(start[1][:, off:off + n])), k
    off, _, n = lay.entries["encoder.topic_fc.weight"]
    assert not torch.equal(fr.eng.master[off:off + n], start[0][off:off + n])


def test_trainer_frozen_decoder():
    """(b) frozen keys keep master, bf16 copy and zero moments bit for bit; every other key moves (but a one-element key whose
    gradient is rounding noise, see below); grad_norm() is the norm of the trainable tensors"""
    tr, batch = _trainer(param_groups=[{"params": "decoder.gpt2.*", "frozen": True}])
    e, lay = tr.eng, tr.eng.layout
    e.refresh_copies()
    start = {"master": e.master.detach().clone(), "bf16": e.wc.clone()}
    for _ in range(2):
        tr.step(batch, stage=3)
    now = _state(tr)
    frozen = [k for k in lay.keys if k.startswith("decoder.gpt2.")]
    assert 0 < len(frozen) < len(lay.keys) and tr.describe_groups()[0]["tensors"] == len(frozen)
    still = []
    for k in lay.keys:
        off, _, n = lay.entries[k]
        sl = slice(off, off + n)
        if k in frozen:
            assert torch.equal(_bits(now["master"][sl]), _bits(start["master"][sl])), k
            assert torch.equal(_bits(now["bf16"][sl]), _bits(start["bf16"][sl])), k
            assert torch.equal(_bits(now["m"][sl]), torch.zeros_like(_bits(now["m"][sl]))), k
            assert torch.equal(_bits(now["v"][sl]), torch.zeros_like(_bits(now["v"][sl]))), k
        elif torch.equal(now["master"][sl], start["master"][sl]):
            still.append(k)
            # a trainable key stands still only where no gradient to speak of reached it: v, a sum of squares, far below eps^2 =
            # 1e-12, so that lr m / (sqrt(v) + eps) is below half an ulp of p (the plain step leaves it as well).  Only the
            # one-element att_matrices.*.bias can be such keys: each shifts the three scores of one softmax alike, so its
            # gradient is a sum that is zero but for rounding.
            assert float(now["v"][sl].max()) < 1e-18 and float(e.grad[sl].abs().max()) / 12.0 < 1e-7, k
    print("trainable keys without any gradient in two steps:", still)
    assert len(still) <= 4 and all(k.startswith("mm_atten_layer.att_matrices.") and k.endswith(".bias") for k in still)
    # the clip norm.  All terms are non-negative, so any summation order is within (chain of roundings) x 2^-24 relative of the
    # exact sum.  Chain, from the launch geometry: a square (1); per grid trip of a lane at most 4 additions and one hand-over to
    # the lane's LDS slot (5 x trips); 3 additions over a lane's four slots, 6 wave steps; in the final kernel ceil(grid / 256)
    # partials per thread, 6 wave steps, 3 waves; then the groups in order (ngroups).  sqrt halves the relative error; sqrt,
    # the division by the row count and the reference's own float64 arithmetic add 3 more roundings.
    total = lay.total
    grid = min(2048, (total // 4 + 1 + 255) // 256)
    trips = -(-((total + 3) // 4) // (grid * 256))
    chain = 1 + 5 * trips + 3 + 6 + -(-grid // 256) + 6 + 3 + tr.groups.ngroups
    g = e.grad.double().cpu()
    live = torch.zeros(total, dtype=torch.bool)
    for k in lay.keys:
        if k not in frozen:
            off, _, n = lay.entries[k]
            live[off:off + n] = True
    ref = math.sqrt(float((g[live] ** 2).sum())) / 12.0
    got = float(tr.grad_norm())
    print("grad_norm %.9g, float64 %.9g, rel err %.3g, chain %d, bound %.3g" % (got, ref, abs(got - ref) / ref, chain, (chain / 2 + 3) * 2.0 ** -24))
    assert ref > 0 and abs(got - ref) <= ref * (chain / 2 + 3) * 2.0 ** -24
    whole = math.sqrt(float((g ** 2).sum())) / 12.0
    assert whole > ref * (1 + 1e-3)                        # (the frozen tensors' gradients would have shown)
    gn = tr.group_grad_norms().tolist()
    assert gn[0] == 0.0 and gn[1] == got


def test_trainer_lr_scale():
    """(c) the decoder at a tenth of the rate: bit-equal on its keys to a plain trainer whose lr is the fp32 product, and on the
    other keys to the plain trainer at the base rate"""
    dec = lambda tr: [k for k in tr.eng.layout.keys if k.startswith("decoder.gpt2.")]
    rest = lambda tr: [k for k in tr.eng.layout.keys if not k.startswith("decoder.gpt2.")]
    tr = _two_steps_against_plain_runs(dict(max_norm=BIG, param_groups=[{"params": "decoder.gpt2.*", "lr_scale": 0.1}]),
                                       [(dict(max_norm=BIG, lr=group_lr(1e-3, 0.1)), dec), (dict(max_norm=BIG), rest)])
    assert tr.current_lr() == 1e-3


def test_trainer_no_decay():
    """(d) weight_decay 0.1 with the no_decay list: biases and LayerNorm tensors as a plain run without decay, the rest as a plain
    run with 0.1"""
    import fnmatch
    nd = lambda tr: [k for k in tr.eng.layout.keys if fnmatch.fnmatchcase(k, "*bias*") or fnmatch.fnmatchcase(k, "*ln_*")]
    rest = lambda tr: [k for k in tr.eng.layout.keys if k not in nd(tr)]
    tr = _two_steps_against_plain_runs(dict(max_norm=BIG, weight_decay=0.1, param_groups=NO_DECAY),
                                       [(dict(max_norm=BIG, weight_decay=0.0), nd), (dict(max_norm=BIG, weight_decay=0.1), rest)])
    d = tr.describe_groups()
    assert d[0]["weight_decay"] == 0.0 and d[1]["weight_decay"] == 0.1 and d[0]["tensors"] == len(nd(tr))


def test_trainer_resume_with_groups():
    """(e) two steps, state_dict, a fresh trainer with the same groups, two more steps = four steps in one go, bit for bit"""
    kw = dict(weight_decay=0.1, warmup_steps=1, total_steps=8,
              param_groups=[{"params": "decoder.gpt2.transformer.h.0.*", "frozen": True}, {"params": "decoder.gpt2.*", "lr_scale": 0.1}] + NO_DECAY)
    one, batch = _trainer(**kw)
    for _ in range(4):
        one.step(batch, stage=3)
    first, _ = _trainer(**kw)
    for _ in range(2):
        first.step(batch, stage=3)
    sd = first.state_dict()
    assert sd["hparams"]["param_groups"] == kw["param_groups"]
    second, _ = _trainer(state={k: v.detach().cpu().clone() for k, v in first.model.state_dict().items()}, **kw)
    second.load_state_dict(sd)
    for _ in range(2):
        second.step(batch, stage=3)
    a, b = _state(one), _state(second)
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
    assert not torch.equal(a["master"], _state(first)["master"])
