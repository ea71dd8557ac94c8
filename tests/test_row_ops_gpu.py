"""The row kernels, one entry at a time, against float64 restatements (csrc/rowops.hip, mmtg_layernorm_fwd_x3 of csrc/x3.hip).

tests/test_ops_gpu.py holds a handful of LayerNorm shapes against fp32 torch with a tolerance that grows with the row count: a
dropped or doubled row passes it, and no case there takes a second sweep, a ragged chunk trip, the one-wave-per-row backward or the
atomic column sum.  Here every case hands ONE entry inputs already rounded to its storage type, starts every output as NaN between
sentinel pads, and compares what the entry wrote with the same operation restated in float64 on the CPU:

  0. the dispatch of mmtg_layernorm_fwd and ln_bwd_impl restated in Python (dtype, cols, rows, alignment, CU count, switches ->
     kernel family, workgroups, sweeps); every backward case asserts the partial-row count the `_partial` entry returns, and the
     row counts around every sweep boundary come from the same restatement;
  1. LayerNorm forward (f32, bf16, the full-wave bf16 build in one and two sweeps, the x3 plane form): y, mean, rstd, every element,
     on random, offset, constant, single-nonzero and large rows;
  2. LayerNorm backward, exact part: integer data, integer mean, power-of-two rstd -- d gamma and d beta bit for bit on top of an
     integer start value, through every build, every sweep edge, 1 .. 9 rows;
  3. LayerNorm backward, rounded part: d(x) with and without the residual gradient, the masked copy as a pure function of the stored
     d(x) and the hash (bit for bit; plane pairs for x3), its column sum, the zero third workspace row;
  4. column sums (mmtg_colsum one-stage, tall, the atomic kernel behind a null workspace, mmtg_colsum_batch): exact on integers,
     random data to the summation bound;
  5. the split-K finish (mmtg_splitk_finish): exact sums, every epilogue, the folded LayerNorm on the values as stored;
  6. the kernels behind the MMTG_LN_* switches, each in a fresh child process, pinned by the partial-row counts.

Every bound is derived where it is defined (U = 2^-24 per fp32 rounding, half an ulp of the storage type for a bf16 store,
n U sum|terms| for a sum of depth n); only the transcendental yardstick of section 5 is measured, and it is the one of
tests/test_gemm_ops_gpu.py (docs/experiments.md, "Row kernels against float64").  The tests without the gpu mark run a float32 CPU
model of each family (same sweep structure and row strides, for 256 and for 8 CUs) through the same bounds on the same inputs -- a
bound the model cannot meet is a wrong derivation -- and require that the model is REJECTED with each of twelve defects planted.
"""
import functools
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # (section 6 runs this file as a script in a child process)
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import _hash_u32  # noqa: E402
import test_gemm_ops_gpu as G  # noqa: E402  (the transcendental yardsticks and their bounds)

gpu = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32
SENT = 1234.0                # sentinel of elements a kernel must leave alone (exact in bf16)
PAD = 64                     # elements in front of and behind every buffer (16-byte aligned for both types)
U = 2.0 ** -24               # unit roundoff of fp32
EPS = 1e-5
SEED = 99                    # dropout seed
MODEL_CUS = (256, 8)
WORST = {}                   # family -> worst err / allowed seen in this process


def _cdiv(a, b):
    return -(-a // b)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _T(bf):
    return BF if bf else F32


def _within(fam, name, got, ref, allow):
    """every element of got within allow of ref (NaN anywhere fails); records the worst err / allowed of the family"""
    err = (got.double() - ref).abs()
    ratio = (err / allow.clamp(min=1e-300)).nan_to_num(nan=float("inf"))
    ok = err <= allow
    w = float(ratio.max()) if ratio.numel() else 0.0
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d/%d outside the bound, first at %s: got %.9g, ref %.9g, allowed %.3g; worst err/allowed %.3g" % (
            name, len(bad), ok.numel(), i, float(got[i]), float(ref[i]), float(allow[i]), w))
    WORST[fam] = max(WORST.get(fam, 0.0), w)
    return w


def _same_bits(name, got, ref):
    if not torch.equal(_bits(got), _bits(ref)):
        bad = (_bits(got) != _bits(ref)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d/%d elements differ in bits, first at %s: got %.9g, expected %.9g" % (
            name, len(bad), got.numel(), i, float(got[i]), float(ref[i])))


class Buf:
    """a device buffer between two sentinel pads; `off` elements shift the payload off its 16-byte alignment"""

    def __init__(self, shape, dtype, data=None, fill=NAN, off=0):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape))
        self.lo = PAD + off
        host = torch.full((self.lo + self.n + PAD,), fill, dtype=dtype)
        self.pads = (_bits(host[:self.lo]).clone(), _bits(host[self.lo + self.n:]).clone())
        if data is not None:
            host[self.lo:self.lo + self.n] = data.reshape(-1).to(dtype)
        self.flat = host.to(DEV)
        self.t = self.flat[self.lo:self.lo + self.n].view(self.shape)

    def cpu(self, name="buffer"):
        host = self.flat.cpu()
        assert torch.equal(_bits(host[:self.lo]), self.pads[0]) and torch.equal(_bits(host[self.lo + self.n:]), self.pads[1]), \
            name + ": the pads around the buffer changed"
        return host[self.lo:self.lo + self.n].view(self.shape).clone()


class HostBuf(Buf):
    """the same on the CPU, for the float32 models"""

    def __init__(self, shape, dtype, data=None, fill=NAN, off=0):
        self.shape = tuple(shape)
        self.t = torch.full(self.shape, fill, dtype=dtype) if data is None else data.to(dtype).clone().view(self.shape)

    def cpu(self, name="buffer"):
        return self.t.clone()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# =====================================================================================================================
# 0. the routes: mmtg_layernorm_fwd and ln_bwd_impl restated
# =====================================================================================================================
FULL_COLS = (512, 768, 1024)


def fwd_route(bf, cols, rows, aligned, cus, env=()):
    """-> (family, workgroups, sweeps) of mmtg_layernorm_fwd"""
    nb4 = _cdiv(rows, 4)
    if bf and "MMTG_LN_V1" not in env and "MMTG_LN_V2" not in env and cols in FULL_COLS and rows >= 2048 and aligned:
        capf = int(env["MMTG_LN_FWD_CAP"]) if "MMTG_LN_FWD_CAP" in env else 6 * cus
        nbf = min(nb4, capf if capf > 0 else 1)
        sweeps = _cdiv(nb4, nbf)
        return "fwd3", _cdiv(nb4, sweeps), sweeps
    return "fwd1", nb4, 1


def bwd_route(bf, cols, rows, aligned, cus, env=(), x3=False):
    """-> (family, workgroups = partial rows, sweeps) of ln_bwd_impl / ln_bwd_x3_impl.  v1 counts 4-row blocks up to 1024, the
    full-wave build 4-row blocks under its cap, the half-wave builds 8-row blocks"""
    nb = min(_cdiv(rows, 4), 1024)
    epc = 8 if bf else 4
    vec = x3 or ("MMTG_LN_V1" not in env and cols % epc == 0 and aligned)
    cap_env = None if x3 or "MMTG_LN_CAP" not in env else int(env["MMTG_LN_CAP"])
    if vec and not x3 and "MMTG_LN_V2" not in env and bf and (cols in (512, 768) or (cols == 1024 and "MMTG_LN_NO1024" not in env)):
        cap = cap_env if cap_env is not None else (2 * cus if cols == 1024 else 3 * cus)
        nb = min(nb, cap)
        sweeps = _cdiv(_cdiv(rows, 4), nb)
        return "full", _cdiv(_cdiv(rows, 4), sweeps), sweeps
    if vec:
        nb = min(nb, cap_env if cap_env is not None else 2 * cus)
        sweeps = _cdiv(_cdiv(rows, 8), nb)
        nc = _cdiv(cols // epc, 32)
        nc = (2 if nc <= 2 else nc) if bf else (4 if nc <= 4 else 6 if nc <= 6 else 8)
        return "half%d" % nc, _cdiv(_cdiv(rows, 8), sweeps), sweeps
    return "v1", nb, _cdiv(_cdiv(rows, 4), nb)


def sweep_edges(route):
    """the row counts around the first sweep boundary of route(rows): one below the last one-sweep count, it, and one to five above"""
    lo, hi = 1, 1 << 22
    assert route(lo)[2] == 1 and route(hi)[2] > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if route(mid)[2] == 1 else (lo, mid)
    return [lo - 1, lo, lo + 1, lo + 2, lo + 3, lo + 4, lo + 5]


EDGE_IDS = ["B-1", "B", "B+1", "B+2", "B+3", "B+4", "B+5"]

# (name, bf16, x3, expected family, widths, x 8 bytes off its alignment): section 3's table
BUILDS = [
    ("bf16-full", True, False, "full", [512, 768, 1024], False),
    ("bf16-half2", True, False, "half2", [8, 248, 256, 264, 504], False),
    ("bf16-half3", True, False, "half3", [520, 760], False),
    ("bf16-half4", True, False, "half4", [776, 1016], False),
    ("bf16-v1-width", True, False, "v1", [4, 12, 260, 772, 1020], False),
    ("bf16-v1-align", True, False, "v1", [768], True),
    ("f32-half4", False, False, "half4", [4, 124, 128, 132, 512], False),
    ("f32-half6", False, False, "half6", [516, 768], False),
    ("f32-half8", False, False, "half8", [772, 1024], False),
    ("x3-half4", False, True, "half4", [8, 504, 512], False),
    ("x3-half6", False, True, "half6", [520, 768], False),
    ("x3-half8", False, True, "half8", [776, 1024], False),
]
BUILD_IDS = [b[0] for b in BUILDS]
SMALL_ROWS = [1, 2, 7, 8, 9]


def _edge_widths(build):
    """the widths a build runs at its sweep edges: its last ragged one (cols / EPC off a multiple of 32) where it has one; all three
    of the full-wave build, whose template arguments and cap change with the width"""
    name, bf, x3, fam, widths, mis = build
    epc = 8 if bf else 4
    ragged = [w for w in widths if (w // epc) % 32]
    return widths if fam == "full" else [(ragged or widths)[-1]]


def test_routes_restated():
    """the restatement against the figures the dispatch code and its comments give"""
    assert fwd_route(True, 768, 5001, True, 256) == ("fwd3", 1251, 1)            # (no second sweep at 5001 rows)
    assert fwd_route(True, 768, 15104, True, 256) == ("fwd3", 1259, 3)           # the training shape: three sweeps
    assert fwd_route(True, 768, 2047, True, 256)[0] == "fwd1" and fwd_route(True, 768, 2048, False, 256)[0] == "fwd1"
    assert fwd_route(True, 1024, 24 * 256 + 1, True, 256) == ("fwd3", 769, 2)
    assert fwd_route(False, 768, 4096, True, 256)[0] == "fwd1"
    assert bwd_route(True, 768, 15104, True, 256) == ("full", 756, 5)
    assert bwd_route(True, 1024, 2049, True, 256) == ("full", 257, 2)
    assert bwd_route(True, 1024, 2049, True, 256, {"MMTG_LN_NO1024": "1"}) == ("half4", 257, 1)
    assert bwd_route(True, 1024, 70, True, 256, {"MMTG_LN_V2": "1"}) == ("half4", 9, 1)
    assert bwd_route(True, 768, 70, True, 256, {"MMTG_LN_CAP": "2"}) == ("full", 2, 9)
    assert bwd_route(False, 768, 70, True, 256, {"MMTG_LN_CAP": "2"}) == ("half6", 2, 5)
    assert bwd_route(False, 768, 70, True, 256, {"MMTG_LN_V1": "1"}) == ("v1", 18, 1)
    assert bwd_route(True, 772, 5000, True, 256) == ("v1", 1024, 2)
    assert bwd_route(False, 1024, 4097, True, 256, x3=True) == ("half8", 257, 2)
    for name, bf, x3, fam, widths, mis in BUILDS:
        for cols in widths:
            for cus in MODEL_CUS:
                assert bwd_route(bf, cols, 9, not mis, cus, x3=x3)[0] == fam, (name, cols)
    assert sweep_edges(lambda r: bwd_route(True, 768, r, True, 256))[1] == 3072
    assert sweep_edges(lambda r: bwd_route(True, 1024, r, True, 256))[1] == 2048
    assert sweep_edges(lambda r: bwd_route(False, 768, r, True, 256))[1] == 4096
    assert sweep_edges(lambda r: bwd_route(True, 772, r, True, 8))[1] == 4096       # v1 does not know the CU count
    assert sweep_edges(lambda r: bwd_route(False, 768, r, True, 8))[1] == 128


# =====================================================================================================================
# shared: inputs
# =====================================================================================================================
def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _randint(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _fwd_rows(rows, cols, bf, shift=0):
    """[rows, cols] in the storage type.  The first and the last six rows of a call hold, by (row + shift) % 6: a random row, a row of
    mean 300 and spread 0.5 (what a one-pass variance gets wrong), a constant row (variance 0), a single nonzero at column 0, one at
    the last column, and a row of large magnitude (1e4 in f32; in bf16 the same values, stored 2^7 apart); random rows between"""
    x = _rand(rows, cols, seed=1000 * cols + rows + shift, scale=2.0)
    for r in list(range(min(rows, 6))) + list(range(max(rows - 6, 0), rows)):
        k = (r + shift) % 6
        if k == 1:
            x[r] = 300.0 + 0.25 * x[r]
        elif k == 2:
            x[r] = 3.25
        elif k == 3:
            x[r] = 0.0
            x[r, 0] = 5.0
        elif k == 4:
            x[r] = 0.0
            x[r, cols - 1] = -5.0
        elif k == 5:
            x[r] = 5e3 * x[r]
    return x.to(_T(bf))


def _gamma_beta(cols):
    return 1.0 + 0.1 * _rand(cols, seed=cols + 1), 0.1 * _rand(cols, seed=cols + 2)


# =====================================================================================================================
# 1. LayerNorm forward
# =====================================================================================================================
def _fwd_reference(x, g, b, bf_out, D):
    """float64 y, mean, rstd of the stored x and what an fp32 evaluation in the kernel's order may be off by.
    D = fp32 additions on the longest path of a row sum (elements per lane + the shuffle levels) + 1 for the division.
      mean: D U mean|x|.    d = x - mean: the mean's error + U |d| -- it does NOT shrink with d: on the offset row (|x| ~ 300,
      |d| ~ 0.5) and on the constant row (d = 0) it is the whole allowance.
      var = mean(d^2): each square moves by 2 |d| e_d + e_d^2, the sum rounds D + 2 times at the size of var.
      rstd = (var + eps)^-1/2: half the relative error of var + eps, 4 U for the addition, the instruction and the store.
      y = d rstd gamma + beta: gamma (rstd e_d + |d| e_rstd), three roundings of the product, one of the sum; a bf16 store
      adds half an ulp of bf16 at |y|."""
    xd, g, b = x.double(), g.double(), b.double()
    mu = xd.mean(-1)
    d = xd - mu[:, None]
    var = (d * d).mean(-1)
    rs = (var + EPS).rsqrt()
    e_mu = D * U * xd.abs().mean(-1)
    e_d = e_mu[:, None] + U * d.abs()
    e_var = (2 * d.abs() * e_d + e_d * e_d).mean(-1) + (D + 2) * U * var
    e_rs = 0.5 * rs * e_var / (var + EPS - e_var).clamp(min=(var + EPS) / 2) + 4 * U * rs
    t = d * rs[:, None] * g
    y = t + b
    e_y = g.abs() * (rs[:, None] * e_d + d.abs() * e_rs[:, None]) + 3 * U * t.abs() + U * y.abs()
    if bf_out:
        e_y = e_y + G._half_ulp(y.abs() + e_y, BF)
    return dict(y=y, mean=mu, rstd=rs, e_y=e_y, e_mean=e_mu + U * mu.abs(), e_rstd=e_rs)


def _fwd_depth(cols, x3=False):
    return (8 * _cdiv(cols, 512) if x3 else 4 * _cdiv(cols, 256)) + 6 + 1


def _check_stats(fam, name, r, mean, rstd):
    return max(_within(fam, name + " mean", mean, r["mean"], r["e_mean"]), _within(fam, name + " rstd", rstd, r["rstd"], r["e_rstd"]))


def _run_fwd(x, g, b, bf, mis, model=None):
    """one mmtg_layernorm_fwd call (or its float32 model) -> y, mean, rstd on the CPU"""
    rows, cols = x.shape
    B_ = HostBuf if model else Buf
    xb, yb = B_(x.shape, _T(bf), x, off=4 if mis else 0), B_(x.shape, _T(bf))
    gb, bb = B_((cols,), F32, g, fill=SENT), B_((cols,), F32, b, fill=SENT)
    mb, rb = B_((rows,), F32), B_((rows,), F32)
    if model:
        model(xb.t, yb.t, gb.t, bb.t, mb.t, rb.t)
    else:
        hip.layernorm_fwd(xb.t, yb.t, gb.t, bb.t, mb.t, rb.t, rows, cols, EPS)
        torch.cuda.synchronize()
        for q, nm in ((xb, "x"), (gb, "gamma"), (bb, "beta")):
            q.cpu(nm)
    return yb.cpu("y"), mb.cpu("mean"), rb.cpu("rstd")


def _model_fwd(route, defect=None, x3=False):
    """float32 model: per-row statistics in two passes, rows visited in the route's sweeps"""
    fam, nb, sweeps = route

    def run(x, y, g, b, mean, rstd):
        rows, cols = x.shape
        xf = x.float()
        own = torch.ones(cols, dtype=torch.bool)
        if defect == "skip_last_vector" and cols % (512 if x3 else 256):
            own[cols - 4:] = False                     # the last 4-column vector of a ragged trip is not summed
        mu = (xf * own).sum(-1) / cols
        d = xf - mu[:, None]
        if defect == "one_pass_variance":
            var = (xf * xf).sum(-1) / cols - mu * mu
        else:
            var = (d * d * own).sum(-1) / (cols - 1 if defect == "divisor_cols_minus_1" else cols)
        rs = 1.0 / (var.clamp(min=0).sqrt() + EPS) if defect == "eps_outside_sqrt" else torch.rsqrt(var + EPS)
        done = torch.ones(rows, dtype=torch.bool)
        if defect == "drop_last_row_of_second_sweep" and sweeps > 1:
            done[min(rows, 2 * nb * 4) - 1] = False
        y[done] = (d * rs[:, None] * g + b).to(y.dtype)[done]
        mean[done], rstd[done] = mu[done], rs[done]
    return run


def _check_fwd(fam, name, x, g, b, bf, y, mean, rstd):
    r = _fwd_reference(x, g, b, bf, _fwd_depth(x.shape[1]))
    return max(_check_stats(fam, name, r, mean, rstd), _within(fam, name + " y", y, r["y"], r["e_y"]))


FWD_WIDTHS = [4, 8, 252, 256, 260, 512, 764, 768, 1020, 1024]
FWD_ROWS = [1, 3, 4, 5, 9]


def _fwd_small_cases():
    """(rows, shift): row counts under six run once per shift so that every row kind appears"""
    return [(rows, s) for rows in FWD_ROWS for s in range(0, 6, rows) if s == 0 or rows < 6]


def _fwd_generic(cols, bf, engine):
    g, b = _gamma_beta(cols)
    w = 0.0
    for rows, shift in _fwd_small_cases():
        x = _fwd_rows(rows, cols, bf, shift)
        model = engine(fwd_route(bf, cols, rows, True, 256)) if engine else None
        w = max(w, _check_fwd("ln_fwd", "fwd %s %dx%d shift %d" % (_T(bf), rows, cols, shift), x, g, b, bf, *_run_fwd(x, g, b, bf, False, model)))
    return w


@gpu
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cols", FWD_WIDTHS)
def test_layernorm_fwd_generic(cols, bf):
    print("worst err / allowed %.3f" % _fwd_generic(cols, bf, None))


def _fwd_tall_rows(cus):
    """(rows, misaligned): the generic route just under the threshold, the full-wave build in one sweep, in a second ragged sweep
    of one row and of five, and the generic kernel again for an x that sits 8 bytes off a 16-byte boundary"""
    full = max(24 * cus, 2048)            # the rows one sweep of the capped grid holds (the build starts at 2048 rows whatever the cap)
    return [(2047, False), (2048, False), (full + 1, False), (full + 5, False), (2048, True)]


TALL_IDS = ["2047", "2048", "24cus+1", "24cus+5", "2048-misaligned"]


def _fwd_tall(cols, which, cus, engine):
    rows, mis = _fwd_tall_rows(cus)[which]
    route = fwd_route(True, cols, rows, not mis, cus)
    # 2048 rows are one sweep wherever the grid cap holds 512 workgroups (86 CUs and more); the two ragged cases are then two sweeps
    sweeps = _cdiv(_cdiv(rows, 4), 6 * cus) if which in (1, 2, 3) else 1
    assert route[0] == ("fwd3" if which in (1, 2, 3) else "fwd1") and route[2] == sweeps, route
    assert which not in (2, 3) or (sweeps >= 2 and route[1] * 4 * sweeps > rows), route        # (some wave idles in the last sweep)
    g, b = _gamma_beta(cols)
    x = _fwd_rows(rows, cols, True, which)
    return _check_fwd("ln_fwd3" if route[0] == "fwd3" else "ln_fwd", "fwd bf16 %dx%d" % (rows, cols), x, g, b, True,
                      *_run_fwd(x, g, b, True, mis, engine(route) if engine else None))


@gpu
@pytest.mark.parametrize("which", range(5), ids=TALL_IDS)
@pytest.mark.parametrize("cols", FULL_COLS)
def test_layernorm_fwd_bf16_tall(cols, which):
    print("worst err / allowed %.3f" % _fwd_tall(cols, which, _cus(), None))


X3_FWD_COLS = [8, 504, 512, 520, 1024]


def _run_fwd_x3(x, g, b, with_xb, model=None):
    rows, cols = x.shape
    ldp = cols + 8
    plane = rows * ldp + 16
    B_ = HostBuf if model else Buf
    xb, pb = B_(x.shape, F32, x), B_((2 * plane,), BF, fill=SENT)
    gb, bb = B_((cols,), F32, g, fill=SENT), B_((cols,), F32, b, fill=SENT)
    mb, rb = B_((rows,), F32), B_((rows,), F32)
    cb = B_(x.shape, BF) if with_xb else None
    if model:
        y, mean, rstd = torch.full(x.shape, NAN), mb.t, rb.t
        model(xb.t, y, gb.t, bb.t, mean, rstd)
        hi = y.to(BF)
        lo = (y - hi.float()).to(BF)
        for k, p in enumerate((hi, lo)):
            torch.as_strided(pb.t, (rows, cols), (ldp, 1), k * plane).copy_(p)
        if with_xb:
            cb.t.copy_(x.to(BF))
    else:
        hip.layernorm_fwd_x3(xb.t, hip.Planes(pb.t, rows, cols, ldp, plane), gb.t, bb.t, mb.t, rb.t, rows, cols, EPS, xb=cb.t if with_xb else None)
        torch.cuda.synchronize()
        xb.cpu("x")
    p = pb.cpu("planes")
    hi, lo = (torch.as_strided(p, (rows, cols), (ldp, 1), k * plane).clone() for k in (0, 1))
    for k in (0, 1):                                    # the padding columns and the gap between the planes keep the sentinel
        torch.as_strided(p, (rows, cols), (ldp, 1), k * plane).fill_(SENT)
    assert bool((p == SENT).all()), "layernorm_fwd_x3 wrote outside the planes' [rows, cols]"
    return hi, lo, mb.cpu("mean"), rb.cpu("rstd"), (cb.cpu("xb") if with_xb else None)


def _check_pair(fam, name, hi, lo, ref, e):
    """the pair hi + lo against ref within e plus what the split itself leaves (lo's own rounding: half an ulp of bf16 at |lo|, and
    |lo| is at most half an ulp of bf16 at the value: up to 2^-16 of it); hi must be a nearest bf16 of hi + lo, i.e. of the fp32
    value the kernel split (a tie may go either way: lo is rounded after hi is chosen)"""
    w = _within(fam, name + " hi + lo", hi.double() + lo.double(), ref, e + G._half_ulp(G._half_ulp(ref.abs() + e, BF), BF))
    ok = lo.double().abs() <= G._half_ulp(hi.double().abs(), BF)
    assert bool(ok.all()), name + ": hi is not the bf16 rounding of hi + lo at %s" % (tuple((~ok).nonzero()[0].tolist()),)
    return w


def _fwd_x3(cols, with_xb, engine):
    g, b = _gamma_beta(cols)
    w = 0.0
    for rows, shift in [(3, 0), (3, 3), (9, 0)]:
        x = _fwd_rows(rows, cols, False, shift)
        hi, lo, mean, rstd, xb = _run_fwd_x3(x, g, b, with_xb, engine(fwd_route(False, cols, rows, True, 256), x3=True) if engine else None)
        r = _fwd_reference(x, g, b, False, _fwd_depth(cols, x3=True))
        name = "fwd x3 %dx%d shift %d" % (rows, cols, shift)
        w = max(w, _check_stats("ln_fwd_x3", name, r, mean, rstd), _check_pair("ln_fwd_x3", name, hi, lo, r["y"], r["e_y"]))
        if with_xb:
            _same_bits(name + " xb", xb, x.to(BF))
    return w


@gpu
@pytest.mark.parametrize("with_xb", [False, True], ids=["planes", "planes+xb"])
@pytest.mark.parametrize("cols", X3_FWD_COLS)
def test_layernorm_fwd_x3(cols, with_xb):
    print("worst err / allowed %.3f" % _fwd_x3(cols, with_xb, None))


# =====================================================================================================================
# 2 + 3. LayerNorm backward
# =====================================================================================================================
BWD_DEPTH = 40       # fp32 additions on the longest path of a row sum: up to 32 elements per lane (half-wave, NC = 8 x 4) + 6 levels + 2


def _sum_depth(route):
    """roundings on the longest path of a column's sum over the rows: the sweeps of a wave, the half-wave fold and the four waves,
    the 16 row lanes of the second stage walking ceil(nb / 16) partial rows each, their 16-term fold, the add onto the start value"""
    fam, nb, sweeps = route
    return sweeps + 5 + _cdiv(nb, 16) + 16 + 1


def _scale(rows, cols, p, stride=None):
    """dropout_scale of csrc/common.h for every element: (fp32 scale, keep) with index row * cols + col"""
    thresh = hip.drop_thresh(p)
    if not thresh:
        return torch.ones(rows, cols), torch.ones(rows, cols, dtype=torch.bool)
    ik = np.float32(4294967296.0 / (4294967296.0 - float(thresh)))
    idx = (np.arange(rows, dtype=np.int64)[:, None] * (stride or cols) + np.arange(cols, dtype=np.int64)[None, :]).astype(np.uint32)
    keep = _hash_u32(np.uint32(SEED), idx) >= np.uint32(thresh)
    return torch.from_numpy(np.where(keep, ik, np.float32(0.0)).astype(np.float32)), torch.from_numpy(keep)


@functools.lru_cache(maxsize=4)
def _bwd_case(bf, cols, rows, exact):
    """the operands of one backward case, rounded to the storage type.  exact: integers |.| <= 8, an integer mean in -3 .. 3, rstd 1 or
    2, gamma = 1 -- xhat, dy xhat and every partial sum are integers below 2^24 in any order.  Otherwise random rows (the second an
    offset row, the third constant) with the statistics of a float64 forward rounded to fp32"""
    T = _T(bf)
    s = 7919 * cols + rows
    if exact:
        x, dy, dres = (_randint(-8, 8, rows, cols, seed=s + k).to(T) for k in range(3))
        mean, rstd = _randint(-3, 3, rows, seed=s + 3), 2.0 ** _randint(0, 1, rows, seed=s + 4)
        gamma = torch.ones(cols)
    else:
        x = _rand(rows, cols, seed=s, scale=2.0)
        if rows > 2:
            x[1] = 300.0 + 0.25 * x[1]
            x[2] = 3.25
        x, dy, dres = x.to(T), _rand(rows, cols, seed=s + 1).to(T), _rand(rows, cols, seed=s + 2).to(T)
        xd = x.double()
        mean = xd.mean(-1).float()
        rstd = (xd.var(-1, unbiased=False) + EPS).rsqrt().float()
        gamma = 1.0 + 0.1 * _rand(cols, seed=s + 5)
    xd, dyd = x.double(), dy.double()
    xh = (xd - mean.double()[:, None]) * rstd.double()[:, None]
    dg = dyd * gamma.double()
    c1, c2 = dg.mean(-1, keepdim=True), (dg * xh).mean(-1, keepdim=True)
    rs = rstd.double()[:, None]
    dx0 = rs * (dg - c1 - xh * c2)
    # d(x) = rstd (dg - c1 - xhat c2) [+ dres] in fp32: xhat carries 2 U, dg one; c1 and c2 are row means of depth BWD_DEPTH over terms
    # that carry 1 and 4 roundings; the bracket rounds each partial result, the product and the sum with dres once more
    e_c1 = (BWD_DEPTH + 2) * U * dg.abs().mean(-1, keepdim=True)
    e_c2 = (BWD_DEPTH + 5) * U * (dg * xh).abs().mean(-1, keepdim=True)
    e0 = rs * (4 * U * (dg.abs() + c1.abs() + (xh * c2).abs()) + e_c1 + xh.abs() * e_c2 + 2 * U * (xh * c2).abs())
    return dict(bf=bf, cols=cols, rows=rows, exact=exact, x=x, dy=dy, dres=dres, mean=mean, rstd=rstd, gamma=gamma,
                dx0=dx0, e0=e0, tg=dyd * xh, tb=dyd)


MODES = {
    # entry, dres, masked copy, p, column sum
    "plain": ("full", False, False, 0.0, False),
    "dres+mask0.1+colsum": ("full", True, True, 0.1, True),
    "mask0.5": ("full", False, True, 0.5, False),
    "copy-p0+colsum": ("full", True, True, 0.0, True),
    "colsum-only": ("full", False, False, 0.0, True),
    "partial": ("partial", False, False, 0.0, False),
    "partial+dres+mask0.1+colsum": ("partial", True, True, 0.1, True),
}
START = (5.0, -7.0, 3.0)     # d gamma, d beta and the column sum accumulate onto these


def _run_bwd(c, mode, x3, mis, route, model=None):
    """one backward entry (or its model) -> what it wrote, on the CPU"""
    entry, use_dres, copy, p, colsum = MODES[mode]
    bf, rows, cols = c["bf"], c["rows"], c["cols"]
    T = _T(bf)
    B_ = HostBuf if model else Buf
    need = min(_cdiv(rows, 4), 1024) * 3 * cols
    xb, dyb = B_((rows, cols), T, c["x"], off=4 if mis else 0), B_((rows, cols), T, c["dy"])
    drb = B_((rows, cols), T, c["dres"]) if use_dres else None
    gb, mb, rb = B_((cols,), F32, c["gamma"], fill=SENT), B_((rows,), F32, c["mean"], fill=SENT), B_((rows,), F32, c["rstd"], fill=SENT)
    dxb, wsb = B_((rows, cols), T), B_((need,), F32)
    copy = copy or x3                                   # the x3 entries always write the plane pair
    cpb = B_((2, rows, cols), BF) if x3 else (B_((rows, cols), T) if copy else None)
    full = entry == "full"
    outs = [B_((cols,), F32, torch.full((cols,), v), fill=SENT) for v in START] if full else [None] * 3
    if full and not colsum:
        outs[2] = None
    if model:
        n = model(c, route, x3, p, dxb.t, cpb.t if cpb else None, wsb.t, [o.t if o else None for o in outs], use_dres, colsum, full)
    else:
        assert need == hip.lib().mmtg_layernorm_bwd_ws(rows, cols)
        a = (dyb.t, xb.t, gb.t, mb.t, rb.t, drb.t if drb else None, dxb.t)
        o = [q.t if q else None for q in outs]
        if x3:
            planes = hip.Planes(cpb.t, rows, cols)
            if full:
                n = hip.layernorm_bwd_x3(*a, o[0], o[1], rows, cols, planes, drop_p=p, drop_seed=SEED, dcolsum=o[2], ws=wsb.t)
            else:
                n = hip.layernorm_bwd_x3_partial(*a, rows, cols, planes, wsb.t, drop_p=p, drop_seed=SEED, want_colsum=colsum)
        elif full:
            n = hip.layernorm_bwd(*a, o[0], o[1], rows, cols, dx_masked=cpb.t if copy else None, drop_p=p, drop_seed=SEED, dcolsum=o[2], ws=wsb.t)
        else:
            n = hip.layernorm_bwd_partial(*a, rows, cols, wsb.t, dx_masked=cpb.t if copy else None, drop_p=p, drop_seed=SEED, want_colsum=colsum)
        torch.cuda.synchronize()
        for q, nm in ((xb, "x"), (dyb, "dy"), (gb, "gamma"), (mb, "mean"), (rb, "rstd")):
            q.cpu(nm)
    return dict(n=n, dx=dxb.cpu("dx"), copy=cpb.cpu("copy") if cpb else None, ws=wsb.cpu("ws"),
                outs=[q.cpu("sum") if q else None for q in outs])


def _rows_sum_model(P, start, defect=None):
    """colsum_rows_block in float32: 16 row lanes stride the rows, their partial sums are folded in lane order, then start + t"""
    M, N = P.shape
    Q = torch.zeros(_cdiv(M, 16) * 16, N)
    Q[:M] = P
    Q = Q.view(-1, 16, N)
    a = torch.zeros(16, N)
    for k in range(Q.shape[0]):
        a += Q[k]
    t = torch.zeros(N)
    for k in range(16):
        if not (defect == "colsum_lane_left_out" and k == 11):
            t = t + a[k]
    return start + t


def _model_bwd(defect=None):
    """float32 model of ln_bwd_kernel / ln_bwd2_kernel / ln_bwd3_kernel + the ordered second stage: a workgroup owns 4 (8) rows of
    every sweep, a wave (half-wave) accumulates its row of every sweep in sweep order, the halves fold, the four waves fold, the
    second stage folds the workgroups' partial rows"""
    def run(c, route, x3, p, dx, cp, ws, outs, use_dres, colsum, full):
        fam, nb, sweeps = route
        rows, cols = c["rows"], c["cols"]
        T = dx.dtype
        R = 8 if fam.startswith("half") else 4
        x, dy, g = c["x"].float(), c["dy"].float(), c["gamma"]
        mu, rs = c["mean"][:, None], c["rstd"][:, None]
        own = torch.ones(cols)
        if defect == "skip_last_vector" and cols % 256:
            own[cols - 4:] = 0.0
        xh = (x - mu) * rs
        dg = dy * g
        c1 = (dg * own).sum(-1, keepdim=True) * np.float32(1.0 / cols)
        c2 = (dg * xh * own).sum(-1, keepdim=True) * np.float32(1.0 / cols)
        o = rs * ((dg - c1) if defect == "no_c2_term" else (dg - c1 - xh * c2))
        if use_dres and defect != "dres_not_added":
            o = o + c["dres"].float()
        done = torch.ones(rows, dtype=torch.bool)
        if defect == "drop_last_row_of_second_sweep" and sweeps > 1:
            done[min(rows, 2 * nb * R) - 1] = False
        dx[done] = o.to(T)[done]
        want = colsum or cp is not None
        scale, _ = _scale(rows, cols, p, cols + 8 if defect == "dropout_index_padded_stride" else None)
        m = ((o if defect == "mask_unrounded" else o.to(T).float()) * scale).to(T)
        if cp is not None:
            if x3:
                hi = m.to(BF)
                cp[0][done], cp[1][done] = hi[done], (m - hi.float()).to(BF)[done]
            else:
                cp[done] = m[done]
        S = nb * R
        part = []
        for q, t in enumerate((dy * xh, dy, m.float())):
            if q == 2 and not want:
                part.append(torch.zeros(nb, cols))
                continue
            t = t * done[:, None]
            Q = torch.zeros(sweeps * S, cols)
            Q[:rows] = t
            Q = Q.view(sweeps, nb, R, cols)
            acc = torch.zeros(nb, R, cols)
            for k in range(sweeps):
                acc += Q[k]
                if defect == "first_row_of_sweep_twice" and q == 0 and k == 1:
                    acc[0, 0] += Q[k, 0, 0]
            if R == 8:
                acc = acc[:, 0::2] + acc[:, 1::2]
            part.append(((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3])
        ws.view(-1)[:nb * 3 * cols] = torch.stack(part, 1).reshape(-1)
        if full:
            for q in range(3):
                if outs[q] is not None:
                    outs[q].copy_(_rows_sum_model(part[q], outs[q].clone()))
        return None if full else nb
    return run


def _check_bwd(fam, name, c, mode, x3, route, out):
    """every output of one backward call against the float64 restatement; returns the worst err / allowed"""
    entry, use_dres, copy, p, colsum = MODES[mode]
    bf, rows, cols, exact = c["bf"], c["rows"], c["cols"], c["exact"]
    T = _T(bf)
    _, nb, sweeps = route
    w = 0.0
    if entry == "partial":
        assert out["n"] == nb, "%s: %d partial rows, the route restated gives %d" % (name, out["n"], nb)
    # d(x)
    ref = c["dx0"] + (c["dres"].double() if use_dres else 0.0)
    e = c["e0"] + 2 * U * ref.abs()
    if bf:
        e = e + G._half_ulp(ref.abs() + e, BF)
    dx = out["dx"]
    w = max(w, _within(fam, name + " dx", dx, ref, e))
    # the masked copy: a pure function of the stored d(x) and the hash
    copy = copy or x3
    scale, keep = _scale(rows, cols, p)
    m = (dx.float() * scale).to(T)
    if copy:
        if x3:
            hi = m.to(BF)
            _same_bits(name + " hi plane", out["copy"][0], hi)
            _same_bits(name + " lo plane", out["copy"][1], (m - hi.float()).to(BF))
        else:
            _same_bits(name + " masked copy", out["copy"], m)
        if p > 0 and rows * cols >= 4096:
            n = rows * cols
            assert abs(float(keep.double().mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), name + ": kept fraction %.4f at p = %g" % (float(keep.double().mean()), p)
    # the sums over the rows: d gamma, d beta [, the column sum of the masked copy as stored]
    n = _sum_depth(route)
    ws = out["ws"].view(-1)
    P = ws[:nb * 3 * cols].view(nb, 3, cols)
    assert bool(torch.isnan(ws[nb * 3 * cols:]).all()), name + ": the workspace behind the partial rows was written"
    want = colsum or copy
    terms = [c["tg"], c["tb"], m.double() if want else None]
    for q, nm in enumerate(("d gamma", "d beta", "column sum")):
        if terms[q] is None:
            assert bool((P[:, 2] == 0).all()), name + ": workspace row 2 must be zeros when neither a column sum nor a copy was asked for"
            continue
        s = terms[q].sum(0)
        if exact and q < 2:
            _same_bits(name + " partial rows of " + nm, P[:, q].double().sum(0).float(), s.float())
        else:
            w = max(w, _within(fam, name + " partial rows of " + nm, P[:, q].double().sum(0), s, (n + (3 if q < 2 else 0)) * U * terms[q].abs().sum(0)))
        if entry == "full" and out["outs"][q] is not None:
            if exact and q < 2:
                _same_bits(name + " " + nm, out["outs"][q], (START[q] + s).float())
            else:
                w = max(w, _within(fam, name + " " + nm, out["outs"][q], START[q] + s, (n + (3 if q < 2 else 0)) * U * (terms[q].abs().sum(0) + abs(START[q]))))
    return w


def _bwd(build, rows, exact, modes, cus, engine=None, env=(), widths=None):
    name, bf, x3, fam, all_widths, mis = build
    w = 0.0
    for cols in widths or all_widths:
        route = bwd_route(bf, cols, rows, not mis, cus, env, x3=x3)
        if not env:
            assert route[0] == fam, (name, cols, route)
        c = _bwd_case(bf, cols, rows, exact)
        for mode in modes:
            nm = "%s %dx%d %s%s" % (name, rows, cols, mode, " exact" if exact else "")
            out = _run_bwd(c, mode, x3, mis, route, engine)
            w = max(w, _check_bwd("ln_bwd_" + route[0] + ("_x3" if x3 else ""), nm, c, mode, x3, route, out))
    return w


EXACT_MODES = ["colsum-only", "partial"]
ROUNDED_MODES_SMALL = list(MODES)
ROUNDED_MODES_EDGE = ["dres+mask0.1+colsum", "partial"]


def _edge_rows(build, cols, cus):
    name, bf, x3, fam, widths, mis = build
    return sweep_edges(lambda r: bwd_route(bf, cols, r, not mis, cus, x3=x3))


def _bwd_edges(build, edges, exact, modes, cus, engine=None):
    return max(_bwd(build, _edge_rows(build, cols, cus)[k], exact, modes, cus, engine, widths=[cols]) for cols in _edge_widths(build) for k in edges)


@gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_layernorm_bwd_exact_small(build):
    cus = _cus()
    print("worst err / allowed %.3f" % max(_bwd(build, rows, True, EXACT_MODES, cus) for rows in SMALL_ROWS))


@gpu
@pytest.mark.parametrize("edge", range(7), ids=EDGE_IDS)
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_layernorm_bwd_exact_sweep_edges(build, edge):
    print("worst err / allowed %.3f" % _bwd_edges(build, [edge], True, EXACT_MODES, _cus()))


@gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_layernorm_bwd_rounded_small(build):
    cus = _cus()
    print("worst err / allowed %.3f" % max(_bwd(build, rows, False, ROUNDED_MODES_SMALL, cus) for rows in SMALL_ROWS))


@gpu
@pytest.mark.parametrize("edge", [1, 2, 6], ids=["B", "B+1", "B+5"])
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_layernorm_bwd_rounded_sweep_edges(build, edge):
    print("worst err / allowed %.3f" % _bwd_edges(build, [edge], False, ROUNDED_MODES_EDGE, _cus()))


# =====================================================================================================================
# 4. column sums
# =====================================================================================================================
CS_M = [1, 15, 16, 17, 127, 128, 129, 255, 257, 2048]
CS_N = [1, 63, 64, 65, 100]
CS_TALL_M = [2049, 2052 + 128]
CS_TALL_N = [4, 252, 256, 260]
CS_START = 9.0


def _cs_data(M, N, ldx, bf, exact, seed=0):
    """[M, ldx] in the storage type; the columns from N on hold NaN (never read)"""
    X = torch.full((M, ldx), NAN)
    X[:, :N] = _randint(-8, 8, M, N, seed=M * 131 + N + seed) if exact else _rand(M, N, seed=M * 131 + N + seed)
    return X.to(_T(bf))


def _cs_route(M, N, ws):
    """-> (path, roundings on the longest path of a column): one stage = 16 row lanes + their fold + the add onto out; tall = 4 row
    lanes over a slice of rpb rows + their fold, then one stage over the slices"""
    if M <= 2048:
        return "rows", _cdiv(M, 16) + 16 + 1
    if ws:
        rpb = (_cdiv(M, 128) + 3) & ~3
        return "slices", _cdiv(rpb, 4) + 4 + _cdiv(_cdiv(M, rpb), 16) + 16 + 1
    rpb = max(16, (_cdiv(M, max(1, 1024 // _cdiv(N, 256))) + 3) & ~3)
    return "atomic", _cdiv(rpb, 4) + 4 + _cdiv(M, rpb)


def _slices_model(X, M, N, rpb):
    out = []
    for r0 in range(0, M, rpb):
        a = torch.zeros(4, N)
        for r in range(r0, min(M, r0 + rpb)):
            a[(r - r0) % 4] += X[r, :N]
        out.append(((a[0] + a[1]) + a[2]) + a[3])
    return torch.stack(out)


def _model_colsum(defect=None):
    def run(X, M, N, out, ws_mode):
        Xf = X.float()
        path, _ = _cs_route(M, N, ws_mode == "ws")
        if path == "rows":
            return _rows_sum_model(Xf[:, :N], out, defect)
        if path == "slices":
            return _rows_sum_model(_slices_model(Xf, M, N, (_cdiv(M, 128) + 3) & ~3), out, defect)
        for s in _slices_model(Xf, M, N, max(16, (_cdiv(M, max(1, 1024 // _cdiv(N, 256))) + 3) & ~3)):
            out = out + s
        return out
    return run


def _run_colsum(X, M, N, bf, ws_mode, model=None):
    """ws_mode: None (one stage), "ws" (tall, with a workspace 64 floats longer than mmtg_colsum_ws), "null" (tall, no workspace)"""
    if model:
        return model(X, M, N, torch.full((N,), CS_START), ws_mode)
    xb, ob = Buf(X.shape, _T(bf), X), Buf((N,), F32, torch.full((N,), CS_START), fill=SENT)
    need = int(hip.lib().mmtg_colsum_ws(M, N))
    assert need == (128 * N if M > 2048 else 0)
    if ws_mode == "ws":
        wsb = Buf((need + 64,), F32)
        hip.colsum(xb.t, M, N, ob.t, ldx=X.shape[1], ws=wsb.t)
    elif ws_mode == "null":
        hip._check(hip.lib().mmtg_colsum(hip.dt(xb.t), xb.t.data_ptr(), X.shape[1], M, N, ob.t.data_ptr(), 0, 0, hip._stream()), "colsum")
    else:
        hip.colsum(xb.t, M, N, ob.t, ldx=X.shape[1])
    torch.cuda.synchronize()
    xb.cpu("X")
    if ws_mode == "ws":
        assert bool(torch.isnan(wsb.cpu("ws")[need:]).all()), "colsum wrote behind mmtg_colsum_ws(M, N) floats of its workspace"
    return ob.cpu("out")


def _check_colsum(name, X, M, N, exact, got, ws_mode):
    ref = CS_START + X[:, :N].double().sum(0)
    if exact:
        _same_bits(name, got, ref.float())
        return 0.0
    path, n = _cs_route(M, N, ws_mode == "ws")
    return _within("colsum_" + path, name, got, ref, n * U * (X[:, :N].double().abs().sum(0) + CS_START))


def _colsum_rows(bf, engine):
    w = 0.0
    for M in CS_M:
        for N in CS_N:
            for exact in ((True, False) if (M, N) in ((2048, 100), (257, 65)) else (True,)):
                X = _cs_data(M, N, N + 3, bf, exact)
                w = max(w, _check_colsum("colsum %s %dx%d" % (_T(bf), M, N), X, M, N, exact, _run_colsum(X, M, N, bf, None, engine), None))
    return w


def _colsum_tall(bf, ws_mode, engine):
    w = 0.0
    for M in CS_TALL_M if ws_mode == "ws" else [2049]:
        for N in CS_TALL_N:
            for exact in ((True, False) if N == 260 else (True,)):
                X = _cs_data(M, N, N + 4, bf, exact)
                w = max(w, _check_colsum("colsum %s %dx%d %s" % (_T(bf), M, N, ws_mode), X, M, N, exact, _run_colsum(X, M, N, bf, ws_mode, engine), ws_mode))
    return w


@gpu
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_colsum_one_stage(bf):
    print("worst err / allowed %.3f" % _colsum_rows(bf, None))


@gpu
@pytest.mark.parametrize("ws_mode", ["ws", "null"], ids=["slices", "atomic"])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_colsum_tall(bf, ws_mode):
    print("worst err / allowed %.3f" % _colsum_tall(bf, ws_mode, None))


BATCH_SIZES = [1, 64, 65]


def _batch_items(n):
    """(M, N) per item, the smallest N first (so the filler items of a short launch, copies of item 0, are narrower than maxn)"""
    Ms = [1, 17, 128, 129, 300, 2048, 16, 33]
    Ns = [1, 63, 64, 65, 100, 130]
    return [(Ms[i % len(Ms)], Ns[(i * 5) % len(Ns)] if i else 1) for i in range(n)]


def _colsum_batch(n, engine):
    items = _batch_items(n)
    exact = [i % 7 != 3 for i in range(n)]
    Xs = [_cs_data(M, N, N + 5, False, ex, seed=i) for i, ((M, N), ex) in enumerate(zip(items, exact))]
    if engine:
        got = [engine(X, M, N, torch.full((N,), CS_START), None) for X, (M, N) in zip(Xs, items)]
    else:
        xb = [Buf(X.shape, F32, X) for X in Xs]
        ob = [Buf((N,), F32, torch.full((N,), CS_START), fill=SENT) for M, N in items]
        hip.colsum_batch([(x.t.data_ptr(), o.t.data_ptr(), X.shape[1], M, N) for x, o, X, (M, N) in zip(xb, ob, Xs, items)])
        torch.cuda.synchronize()
        got = [o.cpu("out of item %d" % i) for i, o in enumerate(ob)]
    return max(_check_colsum("colsum_batch of %d, item %d (%dx%d)" % (n, i, M, N), Xs[i], M, N, exact[i], got[i], None) for i, (M, N) in enumerate(items))


@gpu
@pytest.mark.parametrize("n", BATCH_SIZES)
def test_colsum_batch(n):
    print("worst err / allowed %.3f" % _colsum_batch(n, None))


# =====================================================================================================================
# 5. split-K finish
# =====================================================================================================================
SK_M = 3
SK_N = [4, 1020, 1024, 1028, 2048, 2052, 3072, 3076, 4096]
SK_SPLITS = [1, 2, 5]
SK_EPI = {"none": hip.EPI_NONE, "gelu": hip.EPI_GELU, "tanh": hip.EPI_TANH, "resid": hip.EPI_RESID}


@functools.lru_cache(maxsize=4)
def _sk_data(N, splits):
    """slabs, bias and residual in multiples of 1/16 (every sum is exact in fp32 and stays inside the +-24 the transcendental
    yardsticks of tests/test_gemm_ops_gpu.py were taken on), rows with ldp = N + 8 whose padding is NaN"""
    part = torch.full((splits, SK_M, N + 8), NAN)
    part[:, :, :N] = _randint(-48, 48, splits, SK_M, N, seed=N + splits) / 16
    bias = _randint(-64, 64, N, seed=N + 7) / 16
    aux = _randint(-127, 127, SK_M, N, seed=N + 8) / 16
    g, b = _gamma_beta(N)
    return part, bias, aux, g, b


def _model_splitk(defect=None):
    def run(part, splits, N, bias, epi, aux, bf, g, b, ln):
        a = torch.zeros(SK_M, N)
        for k in range(splits):
            if not (defect == "slab_left_out" and k == splits - 1 and splits > 1):
                a = a + part[k, :, :N]
        if bias is not None:
            a = a + bias
        if epi == "gelu":
            a = a * torch.sigmoid(G._gelu_w(a)) if bf else G._f32_forms(a)["gelu"]
        elif epi == "tanh":
            a = torch.tanh(a)
        elif epi == "resid":
            a = a + aux.to(_T(bf)).float()
        out = a.to(_T(bf))
        lo = None
        if ln:
            v = out.float()
            mu = v.mean(-1, keepdim=True)
            var = ((v - mu) ** 2).mean(-1, keepdim=True)
            lo = ((v - mu) * torch.rsqrt(var + EPS) * g + b).to(_T(bf))
        return out, lo
    return run


def _run_splitk(N, splits, epi, bf, with_bias, ln, model=None):
    part, bias, aux, g, b = _sk_data(N, splits)
    if model:
        return model(part, splits, N, bias if with_bias else None, epi, aux, bf, g, b, ln)
    T = _T(bf)
    ldo, ldaux = N + 4, N + 12
    pb = Buf(part.shape, F32, part)
    bb = Buf((N,), F32, bias, fill=SENT) if with_bias else None
    A = torch.full((SK_M, ldaux), NAN)
    A[:, :N] = aux
    ab = Buf(A.shape, T, A) if epi == "resid" else None
    ob, lb = Buf((SK_M + 1, ldo), T, fill=SENT), (Buf((SK_M + 1, N), T, fill=SENT) if ln else None)
    gb, tb = Buf((N,), F32, g, fill=SENT), Buf((N,), F32, b, fill=SENT)
    hip.splitk_finish(pb.t, splits, SK_M, N, ob.t, bias=bb.t if bb else None, epi=SK_EPI[epi], aux=ab.t if ab else None, ldaux=ldaux,
                      ldp=N + 8, ldo=ldo, ln_gamma=gb.t if ln else None, ln_beta=tb.t if ln else None, ln_out=lb.t if ln else None, eps=EPS)
    torch.cuda.synchronize()
    pb.cpu("slabs")
    o = ob.cpu("out")
    assert bool((o[:SK_M, N:] == SENT).all() and (o[SK_M] == SENT).all()), "splitk_finish wrote outside out's [M, N]"
    lo = None
    if ln:
        lo = lb.cpu("ln_out")
        assert bool((lo[SK_M] == SENT).all()), "splitk_finish wrote behind ln_out's last row"
        lo = lo[:SK_M].clone()
    return o[:SK_M, :N].clone(), lo


def _check_splitk(N, splits, epi, bf, with_bias, ln, out, lo):
    part, bias, aux, g, b = _sk_data(N, splits)
    name = "splitk %s N=%d splits=%d %s%s" % (_T(bf), N, splits, epi, "+bias" if with_bias else "")
    v = part[:, :, :N].double().sum(0) + (bias.double() if with_bias else 0.0)
    assert float(v.abs().max()) <= G.ARG_MAX
    w = 0.0
    if epi in ("none", "resid"):
        if epi == "resid":
            v = v + aux.to(_T(bf)).double()
        assert torch.equal(v.float().double(), v)
        _same_bits(name, out, v.float().to(_T(bf)))          # f32: the value itself; bf16: its round-to-nearest-even
    else:
        ref = G.F64_FORMS[epi](v)
        e = G._fn_err(epi, v, bf)
        e = e + (G._half_ulp(ref.abs() + e, BF) if bf else U * ref.abs())
        w = _within("splitk_" + epi, name, out, ref, e)
    if ln:
        # the statistics are those of the values as stored: normalise the float64 image of the stored out.  Row sums of depth
        # 4 NV elements per thread + 6 shuffle levels + the 4 waves + the division
        r = _fwd_reference(out, g, b, bf, 4 * _cdiv(N, 1024) + 6 + 4 + 1)
        w = max(w, _within("splitk_ln", name + " ln_out", lo, r["y"], r["e_y"]))
    return w


def _sk_cases():
    """(N, splits, epilogue, bias, ln): every N x splits x epilogue, bias and the folded LayerNorm alternating so that each epilogue
    sees both at every N"""
    out = []
    for i, N in enumerate(SK_N):
        for j, splits in enumerate(SK_SPLITS):
            for k, epi in enumerate(SK_EPI):
                out.append((N, splits, epi, (i + j + k) % 2 == 0, (i + j) % 2 == 0))
    return out


def _splitk(N, bf, engine):
    w = 0.0
    for case in [c for c in _sk_cases() if c[0] == N]:
        _, splits, epi, with_bias, ln = case
        w = max(w, _check_splitk(N, splits, epi, bf, with_bias, ln, *_run_splitk(N, splits, epi, bf, with_bias, ln, engine)))
    return w


@gpu
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", SK_N)
def test_splitk_finish(N, bf):
    print("worst err / allowed %.3f" % _splitk(N, bf, None))


def test_splitk_yardstick_float32_cpu():
    """the measured term of section 5: the fp32 forms of common.h on the CPU in float32 against float64 over the arguments the
    split-K cases produce, relative to the scales of tests/test_gemm_ops_gpu.py.  The figures printed here are recorded in
    docs/experiments.md; the assertion is against the allowance the kernels get, LIBM_FACTOR times the GEMM suite's yardsticks"""
    for fn, yard in (("tanh", G.TANH_YARD), ("gelu", G.GELU_YARD)):
        worst = 0.0
        for N in SK_N:
            for splits in SK_SPLITS:
                part, bias, _, _, _ = _sk_data(N, splits)
                for v in (part[:, :, :N].double().sum(0), part[:, :, :N].double().sum(0) + bias.double()):
                    got = G._f32_forms(v.float())[fn].double()
                    scale = dict(tanh=torch.ones_like(v), gelu=v.abs())[fn]
                    worst = max(worst, float(((got - G.F64_FORMS[fn](v)).abs() / scale.clamp(min=1e-30)).max()))
        print("float32 %s against float64 on the split-K arguments: largest error / scale %.3e (yardstick %.3e, allowed %.3e)" % (fn, worst, yard, G.LIBM_FACTOR * yard))
        assert worst <= G.LIBM_FACTOR * yard, (fn, worst)


# =====================================================================================================================
# the float32 CPU models through every bound, and the planted defects
# =====================================================================================================================
def test_model_fwd_meets_every_bound():
    w = max(_fwd_generic(cols, bf, _model_fwd) for cols in FWD_WIDTHS for bf in (False, True))
    w = max(w, max(_fwd_tall(cols, which, 8, _model_fwd) for cols in FULL_COLS for which in range(5)))
    w = max(w, _fwd_tall(768, 3, 256, _model_fwd))
    w = max(w, max(_fwd_x3(cols, xb, _model_fwd) for cols in X3_FWD_COLS for xb in (False, True)))
    print("forward models: worst err / allowed %.3f" % w)


@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_model_bwd_meets_every_bound(build):
    eng = _model_bwd()
    w = 0.0
    for exact, modes in ((True, EXACT_MODES), (False, ROUNDED_MODES_SMALL)):
        w = max(w, max(_bwd(build, rows, exact, modes, 256, eng) for rows in SMALL_ROWS))
    w = max(w, _bwd_edges(build, (1, 2, 6), True, EXACT_MODES, 8, eng), _bwd_edges(build, (1, 2, 6), False, ROUNDED_MODES_EDGE, 8, eng))
    if build[0] in ("bf16-full", "f32-half6"):
        w = max(w, _bwd_edges(build, [6], True, EXACT_MODES, 256, eng), _bwd_edges(build, [6], False, ROUNDED_MODES_EDGE, 256, eng))
    for env in ({"MMTG_LN_CAP": "2"}, {"MMTG_LN_V2": "1"}):
        if build[3] != "v1" and not build[2]:
            w = max(w, _bwd(build, 70, True, EXACT_MODES, 256, eng, env, build[4][-1:]), _bwd(build, 70, False, ROUNDED_MODES_EDGE, 256, eng, env, build[4][-1:]))
    print("%s model: worst err / allowed %.3f" % (build[0], w))


def test_model_colsum_and_splitk_meet_every_bound():
    eng = _model_colsum()
    w = max(_colsum_rows(bf, eng) for bf in (False, True))
    w = max(w, max(_colsum_tall(bf, m, eng) for bf in (False, True) for m in ("ws", "null")))
    w = max(w, max(_colsum_batch(n, eng) for n in BATCH_SIZES))
    w = max(w, max(_splitk(N, bf, _model_splitk()) for N in SK_N for bf in (False, True)))
    print("column sum and split-K models: worst err / allowed %.3f" % w)


def _by(name):
    return next(b for b in BUILDS if b[0] == name)


# defect -> a run of the checks that must reject the model with the defect planted (each passes with defect None: the tests above)
DEFECTS = {
    "one_pass_variance": lambda d: _fwd_generic(512, False, functools.partial(_model_fwd, defect=d)),
    "divisor_cols_minus_1": lambda d: _fwd_generic(1024, False, functools.partial(_model_fwd, defect=d)),
    "eps_outside_sqrt": lambda d: _fwd_generic(768, True, functools.partial(_model_fwd, defect=d)),
    "skip_last_vector": lambda d: _fwd_generic(260, False, functools.partial(_model_fwd, defect=d)),
    "drop_last_row_of_second_sweep": lambda d: _bwd_edges(_by("f32-half6"), [3], True, ["colsum-only"], 8, _model_bwd(d)),
    "first_row_of_sweep_twice": lambda d: _bwd_edges(_by("bf16-full"), [2], True, ["colsum-only"], 8, _model_bwd(d)),
    "no_c2_term": lambda d: _bwd(_by("bf16-half3"), 9, False, ["plain"], 256, _model_bwd(d)),
    "dres_not_added": lambda d: _bwd(_by("bf16-v1-width"), 9, False, ["copy-p0+colsum"], 256, _model_bwd(d)),
    "mask_unrounded": lambda d: _bwd(_by("bf16-half2"), 9, False, ["dres+mask0.1+colsum"], 256, _model_bwd(d)),   # (p = 0.5 scales by 2: exact)
    "dropout_index_padded_stride": lambda d: _bwd(_by("f32-half4"), 9, False, ["mask0.5"], 256, _model_bwd(d)),
    "slab_left_out": lambda d: _splitk(1028, False, _model_splitk(d)),
    "colsum_lane_left_out": lambda d: _colsum_rows(False, _model_colsum(d)),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_rejected(defect):
    with pytest.raises(AssertionError) as info:
        DEFECTS[defect](defect)
    print("%s: rejected with: %s" % (defect, str(info.value)[:200]))


def test_drop_last_row_defect_is_rejected_in_the_forward_too():
    with pytest.raises(AssertionError):
        _fwd_tall(768, 3, 8, functools.partial(_model_fwd, defect="drop_last_row_of_second_sweep"))


def test_case_counts():
    """the tables above, counted: a case that silently left a list would shrink these"""
    assert len(_fwd_small_cases()) * len(FWD_WIDTHS) * 2 == 260 and len(FULL_COLS) * 5 == 15 and len(X3_FWD_COLS) * 2 * 3 == 30
    widths = sum(len(b[4]) for b in BUILDS)
    edge_widths = sum(len(_edge_widths(b)) for b in BUILDS)
    assert (widths, edge_widths) == (34, 14)
    assert widths * len(SMALL_ROWS) * len(EXACT_MODES) + edge_widths * 7 * len(EXACT_MODES) == 536
    assert widths * len(SMALL_ROWS) * len(ROUNDED_MODES_SMALL) + edge_widths * 3 * len(ROUNDED_MODES_EDGE) == 1274
    assert len(CS_M) * len(CS_N) == 50 and len(CS_TALL_M) * len(CS_TALL_N) == 8 and sum(BATCH_SIZES) == 130
    assert len(_sk_cases()) == 108 and len({c[:3] for c in _sk_cases()}) == 108
    for epi in SK_EPI:
        for N in SK_N:
            mine = [c for c in _sk_cases() if c[0] == N and c[2] == epi]
            assert {c[3] for c in mine} == {True, False} == {c[4] for c in mine}, (N, epi)
    assert len(SETTINGS) == 5 and len(DEFECTS) == 12


# =====================================================================================================================
# 6. the kernels behind the switches, each in a fresh child process
# =====================================================================================================================
SETTINGS = {
    "v1": {"MMTG_LN_V1": "1"},
    "v2": {"MMTG_LN_V2": "1"},
    "no1024": {"MMTG_LN_NO1024": "1"},
    "finalize-atomic": {"MMTG_LN_FINALIZE_ATOMIC": "1"},
    "cap2": {"MMTG_LN_CAP": "2", "MMTG_LN_FWD_CAP": "2"},
}
CHILD_BWD = [(True, 512), (True, 768), (True, 1024), (True, 504), (False, 516), (False, 1024)]
CHILD_FWD = [(True, 512), (True, 768), (True, 1024), (False, 768)]
# a child takes a few seconds (import, about 60 small cases); the limit is there only to end a hang
CHILD_LIMIT = 120


def _child_rows(cus):
    return [9, 70, 12 * cus + 5]


def _child_counts(cus, env):
    """the partial-row counts of the child's backward cases under the switches `env`, from the route restated"""
    return {"%s:%d:%d" % ("bf16" if bf else "f32", cols, rows): bwd_route(bf, cols, rows, True, cus, env)[1]
            for bf, cols in CHILD_BWD for rows in _child_rows(cus)}


def _child_main(out_path):
    """a bf16 + f32 subset of sections 1 to 3 through the same references and bounds, on whatever kernels this process's switches
    select; reports the worst err / allowed per family, the partial-row counts and the failures"""
    env = {k: v for k, v in os.environ.items() if k.startswith("MMTG_LN_")}
    cus = _cus()
    report = {"fails": [], "counts": {}, "cases": 0, "cus": cus}
    for bf, cols in CHILD_FWD:
        g, b = _gamma_beta(cols)
        for rows in (9, 2053):
            x = _fwd_rows(rows, cols, bf)
            try:
                _check_fwd("ln_fwd", "fwd %s %dx%d" % (_T(bf), rows, cols), x, g, b, bf, *_run_fwd(x, g, b, bf, False))
            except AssertionError as e:
                report["fails"].append(str(e)[:300])
            report["cases"] += 1
    for bf, cols in CHILD_BWD:
        build = ("child", bf, False, None, [cols], False)
        for rows in _child_rows(cus):
            route = bwd_route(bf, cols, rows, True, cus, env)
            for exact, modes in ((True, EXACT_MODES), (False, ROUNDED_MODES_EDGE)):
                c = _bwd_case(bf, cols, rows, exact)
                for mode in modes:
                    out = _run_bwd(c, mode, False, False, route)
                    if MODES[mode][0] == "partial":
                        report["counts"]["%s:%d:%d" % ("bf16" if bf else "f32", cols, rows)] = out["n"]
                        out["n"] = route[1]          # (the parent compares the counts; the checks go on)
                    try:
                        _check_bwd("ln_bwd_" + route[0], "%s %dx%d %s%s" % (_T(bf), rows, cols, mode, " exact" if exact else ""), c, mode, False, route, out)
                    except AssertionError as e:
                        report["fails"].append(str(e)[:300])
                    report["cases"] += 1
    report["worst"] = WORST
    with open(out_path, "w") as fh:
        json.dump(report, fh)


def test_child_settings_are_told_apart():
    """every switch but the finalize one changes a partial-row count of the child's cases, for 256 CUs and for 8"""
    for cus in MODEL_CUS:
        base = _child_counts(cus, {})
        for name, env in SETTINGS.items():
            assert (_child_counts(cus, env) != base) == (name != "finalize-atomic"), (cus, name)


@gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_layernorm_switches_in_a_child_process(setting, tmp_path):
    """the switches are read once per process, so each setting gets a fresh child (started, never exec'd into; never retried).  A
    child that ends by a signal or at its time limit ends the whole session: nothing more may start on a GPU that has faulted"""
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("MMTG_LN_")}, **SETTINGS[setting])
    out = str(tmp_path / "report.json")
    try:
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        pytest.exit("LayerNorm child process (%s) ran into its time limit of %d s: treated as a hang, nothing more is started" % (setting, CHILD_LIMIT), returncode=3)
    if pr.returncode < 0:
        pytest.exit("LayerNorm child process (%s) ended by signal %d:\n%s" % (setting, -pr.returncode, pr.stderr[-2000:]), returncode=3)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    with open(out) as fh:
        report = json.load(fh)
    print("%s: %d cases, worst err / allowed %s" % (setting, report["cases"], {k: round(v, 3) for k, v in report["worst"].items()}))
    assert report["counts"] == _child_counts(report["cus"], SETTINGS[setting]), "the partial-row counts are not those of " + setting
    assert not report["fails"], "%d failures, first 12:\n" % len(report["fails"]) + "\n".join(report["fails"][:12])
    assert report["cases"] >= 80 and all(v <= 1.0 for v in report["worst"].values()), report["worst"]


@gpu
def test_zz_worst_ratios_per_family():
    """(runs last in this file) the worst err / allowed per kernel family over this process's cases: docs/experiments.md's table"""
    print("CUs %d; worst err / allowed per family: %s" % (_cus(), json.dumps({k: round(v, 3) for k, v in sorted(WORST.items())})))
    assert all(v <= 1.0 for v in WORST.values())


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "child", "usage: test_row_ops_gpu.py child <report.json>"
    _child_main(sys.argv[2])
