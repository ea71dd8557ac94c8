"""mmtg_ema_update and mmtg_swap_f32 alone, against float64 and bit for bit (tests/ema_ref.py holds the formula and the bound).

Sizes: below one 16-byte vector, one vector, a vector and a tail, more than one workgroup-pass of 1024 elements with a tail; and
past the grid of 2048 workgroups x 1024 elements: its last full pass, a scalar tail behind it, a second trip of the grid-stride
loop.  Every buffer sits inside a larger allocation with sentinels on both sides, at an offset of 0 or 1 float: an offset takes
the all-scalar path, which must give the 16-byte path's bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ema_ref import check_update  # noqa: E402
from mmtg_amd import hip  # noqa: E402

DEV = "cuda"
SMALL = [1, 3, 4, 5, 1027]
LARGE = [2097152, 2097155, 2098179]
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 1)]
GUARD = 8
SENTINEL = 0x7FC0BEEF          # a NaN with a payload


def place(bits, off):
    """int32 numpy array -> (whole allocation as int32 device tensor, fp32 view of the data at an offset of `off` floats).  The
    allocation is 16-byte aligned and the data is surrounded by GUARD sentinel words."""
    n = bits.size
    whole = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    assert whole.data_ptr() % 16 == 0
    whole[GUARD + off:GUARD + off + n] = torch.from_numpy(bits.view(np.int32)).to(DEV)
    view = whole[GUARD + off:GUARD + off + n].view(torch.float32)
    assert view.data_ptr() % 16 == 4 * off
    return whole, view


def guards_intact(whole, off, n):
    g = whole.cpu().numpy()
    return bool((g[:GUARD + off] == SENTINEL).all() and (g[GUARD + off + n:] == SENTINEL).all())


def data(n, seed, scale=1.0):
    """ema around `scale`, p = ema + a difference of 1e-7 .. 10 times scale, some elements planted with p == ema -- the first of
    them a -0, as checkpoints hold here and there: its sign is a bit of ema like any other"""
    rng = np.random.default_rng(seed)
    e = (scale * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    if n > 2:
        e[2] = -0.0
    return e, new_p(e, seed + 1, scale)


def new_p(e, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    n = e.size
    p = (e.astype(np.float64) + scale * 10.0 ** rng.uniform(-7.0, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p[2::7] = e[2::7]
    return p


def update(e, p, w, offs=(0, 0), count="none"):
    """one launch on fresh device copies -> the new ema as numpy; p and all sentinels are checked to be untouched"""
    n = e.size
    we, ve = place(e.view(np.int32), offs[0])
    wp, vp = place(p.view(np.int32), offs[1])
    c = None if count == "none" else torch.tensor([count], dtype=torch.float32, device=DEV)
    hip.ema_update(ve, vp, n, w, count=c)
    torch.cuda.synchronize()
    assert guards_intact(we, offs[0], n) and guards_intact(wp, offs[1], n)
    assert (vp.view(torch.int32).cpu().numpy() == p.view(np.int32)).all()          # p is never written
    return ve.cpu().numpy()


# ---- 1
@pytest.mark.parametrize("w", [1e-4, 0.1, 0.9])
@pytest.mark.parametrize("n", SMALL)
def test_three_updates_against_float64(n, w):
    e, p = data(n, seed=n)
    for k in range(3):
        got = update(e, p, w)
        check_update(e, p, w, got, "n = %d, w = %g, update %d" % (n, w, k))
        assert (p[2::7] == e[2::7]).all() and (got.view(np.int32)[2::7] == e.view(np.int32)[2::7]).all()      # the planted elements
        e, p = got, new_p(got, seed=100 * n + k)          # each update is judged alone, on the fp32 state it started from


@pytest.mark.parametrize("n", SMALL)
def test_a_weight_of_zero_keeps_every_bit(n):
    e, p = data(n, seed=n + 50, scale=0.02)
    e[0], p[0] = -0.0, 1.0                  # (0 * 1 + -0 is +0 in the plain expression)
    got = update(e, p, 0.0)
    assert (got.view(np.int32) == e.view(np.int32)).all()
    one = update(e, p, 1.0)
    check_update(e, p, 1.0, one, "n = %d, w = 1" % n)


# ---- 2
@pytest.mark.parametrize("n", SMALL)
def test_the_scalar_path_gives_the_vector_path_s_bits(n):
    e, p = data(n, seed=n + 10, scale=0.02)
    ref = update(e, p, 0.1)
    check_update(e, p, 0.1, ref, "n = %d, |e| ~ 0.02" % n)
    for offs in OFFSETS[1:]:
        got = update(e, p, 0.1, offs)
        assert (got.view(np.int32) == ref.view(np.int32)).all(), (n, offs)


# ---- 3
@pytest.mark.parametrize("n", LARGE)
def test_past_the_grid(n):
    e, p = data(n, seed=3)
    ref = update(e, p, 1e-3)
    check_update(e, p, 1e-3, ref, "n = %d" % n)
    assert (ref[-8:] != e[-8:]).any() and (ref[2097152 - 8:2097152] != e[2097152 - 8:2097152]).any()      # the far end was reached
    for offs in ((1, 0), (0, 1)):
        got = update(e, p, 1e-3, offs)
        assert (got.view(np.int32) == ref.view(np.int32)).all(), (n, offs)


# ---- 4
@pytest.mark.parametrize("n", [5, 1027])
def test_the_count_gates_the_update(n):
    e, p = data(n, seed=n + 20)
    for c in (0.0, -1.0, float("nan")):
        for offs in ((0, 0), (1, 0)):
            got = update(e, p, 0.5, offs, count=c)
            assert (got.view(np.int32) == e.view(np.int32)).all(), (n, c, offs)
    a, b = update(e, p, 0.5, count=7.0), update(e, p, 0.5)
    assert (a.view(np.int32) == b.view(np.int32)).all() and (a != e).any()


# ---- 5
def patterns(n, seed):
    """arbitrary 32-bit patterns with NaNs (payloads), -0 and infinities planted in front"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC01234, 0xFFC0ABCD, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0xFFFFFFFF], dtype=np.uint32)
    k = min(n, special.size)
    bits[:k] = special[:k]
    if n > 16:
        bits[-k:] = special[:k][::-1]
    return bits.view(np.int32)


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: "a+%d,b+%d" % o)
@pytest.mark.parametrize("n", SMALL + LARGE)
def test_swap_exchanges_the_bits(n, offs):
    a, b = patterns(n, seed=n), patterns(n, seed=n + 1)
    wa, va = place(a, offs[0])
    wb, vb = place(b, offs[1])
    hip.swap_f32(va, vb, n)
    torch.cuda.synchronize()
    assert torch.equal(va.view(torch.int32).cpu(), torch.from_numpy(b)) and torch.equal(vb.view(torch.int32).cpu(), torch.from_numpy(a))
    assert guards_intact(wa, offs[0], n) and guards_intact(wb, offs[1], n)          # the floats just beyond n are untouched
    hip.swap_f32(va, vb, n)
    torch.cuda.synchronize()
    assert torch.equal(va.view(torch.int32).cpu(), torch.from_numpy(a)) and torch.equal(vb.view(torch.int32).cpu(), torch.from_numpy(b))
    assert guards_intact(wa, offs[0], n) and guards_intact(wb, offs[1], n)
