"""The dense products against a float64 product of the same integers, exactly, at their tile and stride edges (csrc/gemm.hip).

tests/test_ops_gpu.py compares most GEMM routes with one another bit for bit, and the bf16 routes with an fp32 product under
`helpers.close`, whose absolute term lets whole dropped K elements through (section 3 records that).  Here the operands are small
integers (or small multiples of a power of two): every bf16 x bf16 product and every fp32 partial sum is then exactly representable,
so every kernel's fp32 accumulator must EQUAL the float64 product whatever its K order, split count or reduction tree, and a bf16
store must equal its round-to-nearest-even.  The linear part has no tolerance at all (values are compared as numbers: -0 equals +0):

  1. the case table (data): the routes of mmtg_gemm, each forced by the flags of the ABI, mmtg_gemm_x3 and mmtg_gemm_gather; per
     route a star of shapes around one ragged base shape (every M, every N, every K of the route's lists against the base values of the
     other two, plus one corner with the largest of each) and the route's extra shapes (more items than workgroup slots); the value
     patterns; every case packed and with padded leading dimensions (lda, ldb, ldc, ldaux, ldp wider than the extent by 8, 16, 24,
     32, 40 elements); the refusals;
  2. what is asserted: exact fp32 results, exact round-to-nearest-even bf16 stores, exact epilogues on integer data, the
     transcendental epilogues against the float64 function of an exactly known argument, sentinels around every output and NaN
     around every operand;
  3. the checker checked without a GPU: a CPU restatement of a tiled product (fp32 accumulation over K tiles, K splits, a store through
     the output type) passes every assertion on every case, and is rejected with one defect planted; `helpers.close` at the
     existing tests' shapes accepts the first of those defects and flags 3.6 % of the elements the second one damages;
  4. the kernel cases, one pytest test per (route, layout), the route confirmed by the workgroup records of hip.gemm_trace where the
     kernel writes them (the two-stage 128x128, the persistent 128x128 / 256x128 and the eight-phase kernels; the others must
     leave the trace buffer untouched).

ROWDOT forms delta from the value AS STORED (`(float)(T)v[e] * aux`, gemm_common.h), not from the fp32 accumulator; the reference
does the same, and on `ones` data (|acc| <= K <= 256, exact in bf16) both agree, which test_table_is_sound asserts.  alpha is applied
by the ATOMIC epilogue only (the ABI's definition), so that is where 2.0 and 0.5 are run.  The dropout mask of the RESID epilogue is
hash(seed, m N + n) >= p 2^32 (common.h, the index mmtg_dropout_apply uses on a packed [M, N]); the CPU restatement of the hash is
compared with hip.dropout_apply before it is used.

Bounds of the transcendental epilogues (section 2).  The argument is exact, so there is no K term.  bf16 operands (and the
split-precision product) take the fast forms of common.h, built from v_exp_f32 and v_rcp_f32 (1 ulp each: 2^-23 relative) and fp32
operations (2^-24 each); their error is DERIVED from the forms (_sig_err, _tanh_fast_err, ...).  The fp32 kernels call libm's tanhf: that
term is MEASURED, the error of float32 tanh / gelu_new / gelu_new' on the CPU against float64 over the table's arguments
(test_transcendental_yardsticks prints it) times the project's factor 4.  A bf16-stored value is allowed half an ulp of bf16 at the
reference's magnitude on top, an fp32-stored one half an ulp of fp32.  A band sum is allowed the sum of its 64 elements' bounds
plus 64 2^-24 of the sum of their magnitudes.

Case count (a case = one launch: route, layout, shape, pattern, leading dimensions, epilogue): test_case_counts prints and pins the
figures below.
  f32 NT 186, NN 186, TN 264; regstage NT 254, NN 254, TN 132; no_tr NN 254, TN 132; dma2 NT 288, NN 288, TN 132;
  wide NT 282, NN 282; occ4 NT 288, NN 288, TN 264; persist NT 264, NN 264, TN 136; p256 NT 264, NN 264; skinny NT 288;
  p8-192 NT 216, p8-256 NT 194, p8-288 NT 226, p8-persist NT 6, p8-tn TN 100; x3-192 126, x3-256 98; gather0 68, gather1 132;
  6420 launches in 31 kernel tests, and 16 refusals.  Nothing is skipped on an MI355X.
"""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from helpers import close, rnd, tol

gpu = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 1234.0                # sentinel around every output (exact in bf16)
PAD = 64                     # elements in front of and behind every buffer: 16-byte aligned for every type used
TAIL = 3                     # sentinel rows behind the last row of every output
POISON_ROWS = 256            # NaN rows behind every operand, in the same allocation
EXTRA = dict(a=8, b=16, c=24, aux=32, p=40)      # padded run: ld = extent + EXTRA[...]
U = 2.0 ** -24               # unit roundoff of fp32
DROP_SEED = 77

H = hip
_NS, _NP8 = H.GEMM_NO_SKINNY, H.GEMM_NO_P8


# =====================================================================================================================
# 1. the case table
# =====================================================================================================================
# Per route: the ABI flags that force it, the tile (rows, columns), the K tile bk and the 16-byte chunk ch of its operand type, the
# layouts it is built for, the weight-gradient (TN) epilogues, whether it serves EPI_SPLIT for the K-contiguous layouts ("split"),
# the dGELU column-sum bands ("bands"), ROWDOT ("rowdot"), what it writes into the trace buffer ("trace": one record per workgroup
# -- None: nothing), the K quantum of a split ("kq", default bk), its own M / N / K lists where the defaults do not fit, a CU budget
# for the tile rule (mmtg_gemm_cu_budget), and extra shapes (M, N, K, splits) run with the linear epilogues only.
_DMA = H.GEMM_NO_WIDE | H.GEMM_NO_OCC4 | _NS | _NP8
_P8_M = [1024, 1025, 1151, 1152, 1153, 1279, 1280, 1281]
_K128 = [128, 256, 384, 640]
ROUTES = {
    "f32": dict(dtype=F32, flags=0, tile=(128, 128), bk=32, ch=4, layouts=("NT", "NN", "TN"), tn=("atomic", "split"), split=True,
                bands=True),
    "regstage": dict(flags=H.GEMM_REGSTAGE, tile=(128, 128), layouts=("NT", "NN", "TN"), tn=("atomic",), bands=True),
    "no_tr": dict(flags=H.GEMM_NO_TR, tile=(128, 128), layouts=("NN", "TN"), tn=("atomic",), bands=True),
    "dma2": dict(flags=_DMA, tile=(128, 128), layouts=("NT", "NN", "TN"), tn=("atomic",), split=True, bands=True, rowdot=True,
                 trace=(128, 128)),
    "wide": dict(flags=H.GEMM_WIDE | _NS | _NP8, tile=(192, 128), layouts=("NT", "NN"), split=True, rowdot=True),
    "occ4": dict(flags=H.GEMM_OCC4 | H.GEMM_NO_WIDE | _NS | _NP8, tile=(128, 128), layouts=("NT", "NN", "TN"), tn=("atomic", "split"),
                 split=True, bands=True, rowdot=True),
    # one workgroup gets two items only with more items than the 2 x 256 (256x128: 256) workgroup slots: 3 x 172 = 516 tiles,
    # 3 x 86 = 258 tiles, and for the weight gradient 6 x 7 tiles x 13 K slices = 546 items (the last slice ragged: 824 = 12 x 64 + 56)
    "persist": dict(flags=H.GEMM_PERSIST | H.GEMM_NO_WIDE | _NS | _NP8, tile=(128, 128), layouts=("NT", "NN", "TN"), tn=("atomic",),
                    bands=True, rowdot=True, trace=(128, 128),
                    extra=dict(NT=[(264, 21896, 136, 1)], NN=[(264, 21896, 136, 1)], TN=[(768, 776, 824, 13)])),
    "p256": dict(flags=H.GEMM_P256 | H.GEMM_NO_WIDE | _NS | _NP8, tile=(256, 128), layouts=("NT", "NN"), bands=True, rowdot=True,
                 trace=(256, 128), extra=dict(NT=[(520, 10888, 136, 1)], NN=[(520, 10888, 136, 1)])),
    "skinny": dict(flags=0, tile=(64, 64), layouts=("NT",), split=True, Ms=[1, 7, 8, 9, 63, 64, 65, 137, 256]),
    # eight-phase: M >= 1024, N >= 256, K % 128 == 0.  At these sizes every tile count fits one round of the CUs, where the rule takes
    # 192 rows; with a budget of 10 CUs and N > 256 (two tile columns) 256-row tiles are the ones that fit one round up to M = 1280
    # (5 x 2 = 10 tiles against 7 x 2 = 14 of 192 rows), so M = 1281 (12 tiles) and three tile columns (N = 520: two rounds either
    # way, where 192 rows are cheaper) are left to the other two routes.
    "p8-192": dict(flags=H.GEMM_P8, tile=(192, 256), bk=128, layouts=("NT",), rowdot=True, trace=(192, 256), Ms=_P8_M,
                   Ns=[256, 264, 504, 512, 520], Ks=_K128, base=(1025, 264, 256)),
    "p8-256": dict(flags=0, budget=10, tile=(256, 256), bk=128, layouts=("NT",), bands=True, rowdot=True, trace=(256, 256), Ms=_P8_M[:-1],
                   Ns=[264, 504, 512], Ks=_K128, base=(1025, 264, 256)),
    "p8-288": dict(flags=H.GEMM_P8_288, tile=(288, 256), bk=128, layouts=("NT",), rowdot=True, trace=(288, 256), Ms=_P8_M + [1441],
                   Ns=[256, 264, 504, 512, 520], Ks=_K128, base=(1025, 264, 256)),
    # persistent form: more tiles than CUs -- 22 x 17 = 374 tiles of 192 rows (it writes no trace records)
    "p8-persist": dict(flags=H.GEMM_P8 | H.GEMM_PERSIST, tile=(192, 256), bk=128, layouts=("NT",), Ms=[], Ns=[], Ks=[], base=None,
                       extra=dict(NT=[(4200, 4104, 128, 1)])),
    "p8-tn": dict(flags=H.GEMM_P8, tile=(256, 256), bk=128, kq=128, layouts=("TN",), tn=("split",), trace=(256, 256),
                  Ms=[256, 264, 504, 512, 520], Ns=[256, 264, 520], Ks=_K128, base=(264, 264, 256)),
    # split precision: the rule takes 192 rows wherever the tiles fit one round; with a budget of 8 CUs and one tile column,
    # M = 1537 .. 2048 is 9 .. 11 tiles of 192 rows (two rounds) and 7 .. 8 of 256 rows (one round).  The extra shape meets the
    # rule without a budget on 256 CUs: 17 x 16 = 272 tiles of 192 rows, 13 x 16 = 208 of 256 rows.
    "x3-192": dict(api="x3", tile=(192, 256), bk=128, layouts=("NT",), rowdot=True, trace=(192, 256), Ms=[1, 7, 8, 9, 191, 192, 193, 393],
                   Ns=[8, 248, 256, 264], Ks=_K128, base=(193, 264, 256)),
    "x3-256": dict(api="x3", budget=8, tile=(256, 256), bk=128, layouts=("NT",), bands=True, rowdot=True, trace=(256, 256),
                   Ms=[1537, 1791, 1792, 1793, 2048], Ns=[8, 248, 256], Ks=_K128, base=(1793, 248, 256),
                   extra=dict(NT=[(3080, 4088, 128, 1)]), extra_budget=0),
    "gather0": dict(api="g0", tile=(128, 128), layouts=("NT",), Ks=[64, 128, 192, 384], base=(129, 136, 128)),
    "gather1": dict(api="g1", tile=(128, 128), layouts=("TN",), tn=("split",), base=(136, 136, 136)),
}
for _r in ROUTES.values():
    _r.setdefault("api", "gemm")
    _r.setdefault("dtype", BF)
    _r.setdefault("bk", 64)
    _r.setdefault("ch", 8)
    _r.setdefault("flags", 0)
TESTS = [(route, layout) for route, r in ROUTES.items() for layout in r["layouts"]]
TABLE_ROWS = 37              # rows of the gathered table (mmtg_gemm_gather)

Stage = collections.namedtuple("Stage", "route layout M N K pattern pad")      # operands as staged in memory
Run = collections.namedtuple("Run", "epi f32 splits alpha")                      # one launch on a stage

PATTERNS2 = ("coded", "ones", "ties")          # the second pattern of shape i is PATTERNS2[i % 3]; the first is always ints3
# epilogue -> (value pattern, fp32 output as well?)
EPILOGUES = collections.OrderedDict([
    ("bias", ("ints3", True)), ("bias1", ("ones", False)), ("gelu", ("sixteenths", True)), ("gelu_grad", ("sixteenths", False)),
    ("tanh", ("sixteenths", True)), ("resid", ("ones", False)), ("resid_drop", ("ints3", True)), ("dgelu", ("ints3", True)),
    ("dgelu_bands", ("ints3", False)), ("dgelu_saved", ("ints3", False)), ("dtanh", ("ints3", False)), ("rowdot", ("ones", False)),
    ("rowdot3", ("ints3", False)),
])
X3_EPILOGUES = ["bias", "gelu", "tanh", "resid", "resid_drop", "dgelu", "dgelu_bands", "dtanh", "rowdot"]
G0_EPILOGUES = ["none", "bias", "tanh", "tanh_add"]


def _cdiv(a, b):
    return -(-a // b)


def _kper(K, splits, kq):
    return _cdiv(_cdiv(K, splits), kq) * kq


def _split_counts(K, kq):
    """1, a count whose last slice is ragged, and a count with cdiv(K, kper) < splits (slabs past the end)"""
    out = [1]
    for s in range(2, 9):
        kp = _kper(K, s, kq)
        if _cdiv(K, kp) == s and K % kp:
            out.append(s)
            break
    for s in range(2, 12):
        if _cdiv(K, _kper(K, s, kq)) < s:
            out.append(s)
            break
    return out


def _shapes(route, layout):
    """[(M, N, K, kind)]: the star around the base shape ("m" / "n" / "k": which list the shape comes from), the corner, the
    epilogue shapes ("epi") and the route's extra shapes ("extra")"""
    r = ROUTES[route]
    tm, tn = r["tile"]
    bk, ch = r["bk"], r["ch"]
    tnl = layout == "TN"
    k128 = bk == 128
    Ms = r.get("Ms", [8, tm - 8, tm, tm + 8, 2 * tm + 8] if tnl else [1, 7, 8, 9, tm - 1, tm, tm + 1, 2 * tm + 9])
    Ns = r.get("Ns", [8, tn - 8, tn, tn + 8])
    Ks = r.get("Ks", ([1] if tnl else []) + [ch, bk - ch, bk, bk + ch, 2 * bk + ch, 5 * bk + ch])
    base = r.get("base", (tm + 8 if tnl else tm + 1, tn + 8, 2 * bk + ch))
    out = []
    if base:
        M0, N0, K0 = base
        out += [(M, N0, K0, "m") for M in Ms] + [(M0, N, K0, "n") for N in Ns] + [(M0, N0, K, "k") for K in Ks]
        out.append((Ms[-1], Ns[-1], Ks[-1], "corner"))
        if not tnl and r["api"] != "g0":
            # epilogues: all ragged; whole 64-column heads (ROWDOT) with more than 256 rows; and, where legal, fewer than 16 rows
            me = max(Ms[-1], 2 * tm + 9)
            if r.get("Ms") and max(r["Ms"]) <= 256:
                me = r["Ms"][-2]
            out.append((me, Ns[-1], K0, "epi"))
            out.append((me if me > 256 or max(Ms) <= 256 else 257, (tn if tn >= 128 else 128) + 64, Ks[0] if k128 else bk, "epi"))
            if Ms[0] < 16 and Ns[0] == 8:
                out.append((9, 8, Ks[0] if k128 else ch, "epi"))
        if r["api"] == "g0":
            out.append((Ms[-1], Ns[-1], K0, "epi"))
    out += [(M, N, K, "extra%d" % s) for (M, N, K, s) in r.get("extra", {}).get(layout, [])]
    seen, uniq = set(), []
    for s in out:
        if s[3] in ("m", "n", "k", "corner") and s[:3] in seen:
            continue
        seen.add(s[:3])
        uniq.append(s)
    return uniq


def _runs(route, layout, M, N, K, kind):
    """[(pattern, Run)] of one shape"""
    r = ROUTES[route]
    api = r["api"]
    kq = r.get("kq", r["bk"])
    both = r["dtype"] == BF and api == "gemm"          # bf16 operands: a bf16 and an fp32 output
    runs = []
    if kind == "epi":
        if api == "g0":
            return [("sixteenths" if e.startswith("tanh") else "ints3", Run(e, False, 1, 1.0)) for e in G0_EPILOGUES]
        for e, (pat, f32too) in EPILOGUES.items():
            if api == "x3" and e not in X3_EPILOGUES:
                continue
            if e.startswith("rowdot") and not (r.get("rowdot") and M > 256 and N % 64 == 0):
                continue
            if e == "dgelu_bands" and not r.get("bands"):
                continue
            if api == "x3":
                pat = {"ints3": "x3a", "ones": "ones", "sixteenths": "sixteenths"}[pat]
            runs.append((pat, Run(e, not both, 1, 1.0)))
            if both and f32too:
                runs.append((pat, Run(e, True, 1, 1.0)))
        return runs
    if kind.startswith("extra"):
        s = int(kind[5:])
        pats = ["x3a", "x3b"] if api == "x3" else ["ints3", "coded"]
        if layout == "TN":
            return [(p, Run(r["tn"][0], True, s, 1.0)) for p in pats]
        return [(p, Run("none", f, 1, 1.0)) for p in pats for f in ((False, True) if both else (True,))][:3]
    idx = [s[:3] for s in _shapes(route, layout)].index((M, N, K))
    if api == "x3":
        pats = ["x3a", "x3b"]
    else:
        pats = ["ints3", PATTERNS2[idx % 3]]
    for pi, p in enumerate(pats):
        if layout == "TN":
            for e in r["tn"]:
                for si, s in enumerate(_split_counts(K, kq) if kind in ("k", "corner") else [1, 2]):
                    runs.append((p, Run(e, True, s, (2.0, 0.5)[(si + pi) % 2] if e == "atomic" else 1.0)))
        elif api == "g0":
            runs.append((p, Run("none", False, 1, 1.0)))
        else:
            runs.append((p, Run("none", not both, 1, 1.0)))
            if both:
                runs.append((p, Run("none", True, 1, 1.0)))
            if r.get("split") and kind in ("k", "corner") and pi == 0:
                runs += [(p, Run("split", True, s, 1.0)) for s in _split_counts(K, kq)]
    if layout != "TN" and api in ("gemm", "x3") and kind in ("m", "n"):
        # the epilogue's own row and column guards (bias and aux vectors, the aux row clamped at M - 1) at every M and N edge
        runs.append(("ones", Run("resid", not both, 1, 1.0)))
    return runs


def _cases(route, layout):
    """every launch of one (route, layout): [(Stage, [Run])], packed and padded"""
    out = []
    for M, N, K, kind in _shapes(route, layout):
        by_pat = collections.OrderedDict()
        for p, run in _runs(route, layout, M, N, K, kind):
            by_pat.setdefault(p, []).append(run)
        for p, rs in by_pat.items():
            for pad in (False, True):
                out.append((Stage(route, layout, M, N, K, p, pad), rs, kind))
    return out


# Combinations the ABI refuses: (what, keyword arguments of _refused, the error text).  They are asserted, not skipped.
REFUSALS = [
    ("ROWDOT at M <= 256", dict(M=256, N=128, K=64, epi="rowdot"), "ROWDOT epilogue needs"),
    ("ROWDOT on the skinny route", dict(M=512, N=128, K=64, epi="rowdot", flags=H.GEMM_SKINNY), "ROWDOT epilogue needs"),
    ("SPLIT with GEMM_PERSIST", dict(M=64, N=128, K=64, epi="split", flags=H.GEMM_PERSIST), "the split epilogue stores raw fp32"),
    ("SPLIT with GEMM_REGSTAGE (bf16)", dict(M=64, N=128, K=64, epi="split", flags=H.GEMM_REGSTAGE), "the split epilogue stores raw fp32"),
    ("K no multiple of 8 (NT, bf16)", dict(M=64, N=128, K=12), "contiguous extent of A"),
    ("K no multiple of 4 (NT, fp32)", dict(M=64, N=128, K=6, dtype=F32), "contiguous extent of A"),
    ("M = 1 for the weight gradient", dict(layout="TN", M=1, N=128, K=64, epi="atomic"), "contiguous extent of A"),
    ("M = 7 for the weight gradient", dict(layout="TN", M=7, N=128, K=64, epi="atomic"), "contiguous extent of A"),
    ("M = 9 for the weight gradient", dict(layout="TN", M=9, N=128, K=64, epi="atomic"), "contiguous extent of A"),
    ("N no multiple of 8 (NN)", dict(layout="NN", M=64, N=12, K=64), "contiguous extent of B"),
    ("dGELU bands on 192x128 tiles", dict(M=512, N=128, K=64, epi="dgelu_bands", flags=H.GEMM_WIDE), "no 192x128 configuration"),
    ("ATOMIC outside the weight gradient", dict(M=64, N=128, K=64, epi="atomic"), "atomic epilogue belongs"),
    ("weight gradient without ATOMIC / SPLIT", dict(layout="TN", M=64, N=128, K=64), "weight-gradient layout has the atomic"),
    ("split precision at K = 64", dict(api="x3", M=64, N=128, K=64), "gemm_x3: K % 128 == 0"),
    ("gather forward at K = 72", dict(api="g0", M=64, N=128, K=72), "forward needs K % 64 == 0"),
    ("gather weight gradient at M = 12", dict(api="g1", M=12, N=128, K=64), "weight gradient writes MMTG_EPI_SPLIT slabs"),
]


# ---------------------------------------------------------------------------------------------------------------- values
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@functools.lru_cache(maxsize=3)
def _values(M, N, K, pattern):
    """a [M, K], b [K, N], acc = a b in float64 (exact: asserted), per pattern"""
    g = _gen(M, N, K, pattern)
    if pattern == "ints3":
        a, b = _ints((M, K), -3, 3, g), _ints((K, N), -3, 3, g)
    elif pattern == "ones":
        a, b = _ints((M, K), -1, 1, g), _ints((K, N), -1, 1, g)
    elif pattern == "ties":                     # results of a few hundred: many exactly half-way between two bf16 values
        a, b = _ints((M, K), -15, 15, g), _ints((K, N), -15, 15, g)
    elif pattern == "sixteenths":               # a small argument for the transcendental epilogues: multiples of 1 / 4, products exact
        a, b = _ints((M, K), -1, 1, g), _ints((K, N), -1, 1, g) / 4.0
    elif pattern == "coded":                    # A selects: C[m, :] = B[m mod K, :], and B's values say where they come from
        a = torch.zeros(M, K, dtype=F64)
        a[torch.arange(M), torch.arange(M) % K] = 1.0
        b = ((torch.arange(K)[:, None] * N + torch.arange(N)[None, :]) % 251 - 125).double()
    elif pattern in ("x3a", "x3b"):             # one operand needs both planes (up to 4095), the other has an empty lo plane
        big, small = (-4095, 4095), (-3, 3)
        ra, rb = (big, small) if pattern == "x3a" else (small, big)
        a, b = _ints((M, K), ra[0], ra[1], g), _ints((K, N), rb[0], rb[1], g)
    else:
        raise KeyError(pattern)
    # every partial sum, in any order, is bounded by K max|a| max|b|: below 2^24 it is an fp32 integer (multiple of 1 / 4)
    assert K * float(a.abs().max()) * float(b.abs().max()) * (4 if pattern == "sixteenths" else 1) < 2 ** 24, (M, N, K, pattern)
    return a, b, a @ b


def _grid(shape, choices, g):
    c = torch.tensor(choices, dtype=F64)
    return c[torch.randint(0, len(choices), shape, generator=g)]


def _side(st, run):
    """the epilogue's own operands in float64: bias [N], aux [M, N], prefill [M, N], keep [M, N]"""
    M, N = st.M, st.N
    g = _gen(M, N, st.K, run.epi, "side")
    e = run.epi
    x = {}
    if e in ("bias", "bias1", "resid", "resid_drop"):
        x["bias"] = _ints((N,), -3, 3, g)
    if e in ("gelu", "gelu_grad", "tanh", "tanh_add"):
        x["bias"] = _ints((N,), -4, 4, g) / 4.0
    if e in ("resid", "resid_drop"):
        x["aux"] = _ints((M, N), -3, 3, g)
    if e in ("dtanh", "dgelu_saved"):
        x["aux"] = _grid((M, N), [0.0, 0.5, -0.5, 1.0, -1.0], g)
    if e in ("dgelu", "dgelu_bands"):
        x["aux"] = _ints((M, N), -16, 16, g) / 4.0
    if e in ("rowdot", "rowdot3"):
        x["aux"] = _ints((M, N), -1, 1, g)
    if e == "tanh_add":
        x["aux_table"] = _ints((11, N), -4, 4, g) / 4.0
        x["aux_rows"] = torch.randint(0, 11, (M,), generator=g, dtype=torch.int32)
        x["aux"] = x["aux_table"][x["aux_rows"].long()]
    if e == "atomic":
        x["prefill"] = _ints((M, N), -3, 3, g)
    if e == "resid_drop":
        x["keep"] = _keep_mask(DROP_SEED, M, N)
    return x


def _keep_mask(seed, M, N, p=0.5):
    """common.h hash_u32 / dropout_scale restated: keep iff hash(seed, m N + n) >= p 2^32"""
    m32 = np.uint64(0xFFFFFFFF)
    idx = (np.arange(M * N, dtype=np.uint64)) & m32
    h = (idx * np.uint64(0x9E3779B1) + np.uint64(seed)) & m32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m32
    h ^= h >> np.uint64(16)
    return torch.from_numpy((h >= np.uint64(hip.drop_thresh(p))).reshape(M, N).copy()).double()


# =====================================================================================================================
# 2. the float64 references and the bounds
# =====================================================================================================================
_K0 = 0.7978845608028654
_A0 = 0.044715


def _gelu_w(x):
    """2 u = 2 k (x + a x^3): gelu_new(x) = x sigmoid(2 u)"""
    return 2.0 * _K0 * (x + _A0 * x ** 3)


def _gelu64(x):
    return x * torch.sigmoid(_gelu_w(x))


def _gelu_grad64(x):
    s = torch.sigmoid(_gelu_w(x))
    return s * (1.0 + x * (1.0 - s) * (2.0 * _K0 + 6.0 * _K0 * _A0 * x * x))


def _sig_err(w, nround):
    """relative error of s = rcp(1 + exp2(t)) with t = -w log2 e formed by `nround` fp32 roundings (constants included).  The
    exponent is off by nround U |t|, which moves E = 2^t by nround U |t| ln 2 = nround U |w| relative; v_exp_f32 adds 2 U; the sum
    1 + E is off by E / (1 + E) = 1 - s of E's error plus its own rounding U; v_rcp_f32 adds 2 U."""
    return torch.sigmoid(-w) * (nround * U * w.abs() + 2 * U) + 3 * U


def _gelu_fast_err(x):
    """gelu_new_t<bf16> = x s: nine roundings on the exponent (c0 = 2 k log2 e from two rounded constants and two products, c1 = c0 a
    from one more of each, x^2, c1 x^2, the sum, the product with x), then one product"""
    return _gelu64(x).abs() * (_sig_err(_gelu_w(x), 9) + U) + 1e-30


def _gelu_grad_fast_err(x):
    """gelu_new_grad_t<bf16> = s (1 + x (1 - s) q), q = 2 k + 6 k a x^2: ds = s rel(s) goes through d/ds = 1 + x q (1 - 2 s); the six
    further operations (1 - s, q's product and sum, two products, the sum with 1, the product with s) each round a partial result
    no larger than s + |x| s (1 - s) q"""
    s = torch.sigmoid(_gelu_w(x))
    q = 2.0 * _K0 + 6.0 * _K0 * _A0 * x * x
    return s * _sig_err(_gelu_w(x), 9) * (1.0 + x * q * (1.0 - 2.0 * s)).abs() + 7 * U * (s + x.abs() * s * (1.0 - s) * q) + 1e-30


def _tanh_fast_err(x):
    """tanh_t<bf16> = 1 - 2 r, r = rcp(1 + exp2(x c)), c = 2 log2 e (one rounded constant, one product: two roundings on the
    exponent, w = -2 x); 2 r is exact, the subtraction rounds the result"""
    r = torch.sigmoid(-2.0 * x)
    return 2.0 * r * _sig_err(-2.0 * x, 2) + U * torch.tanh(x).abs() + 1e-30


# The measured term (fp32 kernels: libm's tanhf): the largest error of the float32 form on the CPU against float64 over the
# arguments the table produces (multiples of 1 / 16 up to +-24: test_table_is_sound asserts the range), relative to the scale below;
# the kernels are allowed LIBM_FACTOR times it.  test_transcendental_yardsticks prints the figures these constants come from.
ARG_MAX = 24.0
LIBM_FACTOR = 4.0
TANH_YARD = 3.0e-8           # absolute
GELU_YARD = 7.5e-8           # of |x|  (0.5 x (1 + tanh): the rounding of 1 + tanh is relative to 1, not to the small sum)
GELU_GRAD_YARD = 5.0e-8      # of 1 + x^2


def _f32_forms(x32):
    """common.h's fp32 forms in float32 torch arithmetic"""
    k, a = torch.tensor(_K0, dtype=F32), torch.tensor(_A0, dtype=F32)
    x2 = x32 * x32
    t = torch.tanh(k * (x32 + a * x32 * x2))
    return dict(tanh=torch.tanh(x32), gelu=0.5 * x32 * (1.0 + t),
                gelu_grad=0.5 * (1.0 + t) + 0.5 * x32 * (1.0 - t * t) * k * (1.0 + 3.0 * a * x2))


def _libm_err(fn, x):
    scale = dict(tanh=torch.ones_like(x), gelu=x.abs(), gelu_grad=1.0 + x * x)[fn]
    return LIBM_FACTOR * dict(tanh=TANH_YARD, gelu=GELU_YARD, gelu_grad=GELU_GRAD_YARD)[fn] * scale + 1e-30


F64_FORMS = dict(tanh=torch.tanh, gelu=_gelu64, gelu_grad=_gelu_grad64)
FAST_ERR = dict(tanh=_tanh_fast_err, gelu=_gelu_fast_err, gelu_grad=_gelu_grad_fast_err)


def _fn_err(fn, x, fast):
    return FAST_ERR[fn](x) if fast else _libm_err(fn, x)


def _half_ulp(x, dtype):
    """half the spacing of dtype at magnitude x >= 0 (float64): x = m 2^e with m in [0.5, 1) has spacing 2^(e - bits)"""
    _, e = torch.frexp(x)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - (9 if dtype == BF else 25)), torch.zeros_like(x))


def _rne(x, dtype):
    """float64 -> fp32 (exact for every value compared exactly: asserted) -> dtype, round to nearest even, back to float64"""
    return x.float().to(dtype).double()


def _slices(K, splits, kq):
    kp = _kper(K, splits, kq)
    return [(min(K, s * kp), min(K, (s + 1) * kp)) for s in range(splits)]


def _types(st, run):
    r = ROUTES[st.route]
    T = r["dtype"]
    x3 = r["api"] == "x3"
    c = F32 if (run.f32 or T == F32 or x3 or run.epi in ("atomic", "split")) else BF
    return dict(C=c, aux2=F32 if x3 else T, T=F32 if x3 else T)


def _expect(st, run, v, side):
    """[(output, ref float64 [rows, cols], bound or None = exact)] of one launch.  v = (a, b, acc)"""
    a, b, acc = v
    r = ROUTES[st.route]
    ty = _types(st, run)
    fast = r["dtype"] == BF or r["api"] == "x3"
    e = run.epi
    pre = acc + side["bias"] if "bias" in side else acc
    aux = side.get("aux")
    out = []
    if e in ("none", "bias", "bias1"):
        out.append(("C", pre, None))
    elif e in ("gelu", "gelu_grad"):
        assert float(pre.abs().max()) <= ARG_MAX
        if e == "gelu":
            out.append(("aux2", pre, None))
        else:
            out.append(("aux2", _gelu_grad64(pre), _fn_err("gelu_grad", pre, fast)))
        out.append(("C", _gelu64(pre), _fn_err("gelu", pre, fast)))
    elif e in ("tanh", "tanh_add"):
        arg = pre + aux if e == "tanh_add" else pre
        assert float(arg.abs().max()) <= ARG_MAX
        out.append(("C", torch.tanh(arg), _fn_err("tanh", arg, fast)))
    elif e == "resid":
        out.append(("C", pre + aux, None))
    elif e == "resid_drop":
        out.append(("C", pre * side["keep"] * 2.0 + aux, None))
    elif e in ("dgelu", "dgelu_bands"):
        gp = _gelu_grad64(aux)
        ref = acc * gp
        bound = acc.abs() * _fn_err("gelu_grad", aux, fast) + U * ref.abs()
        out.append(("C", ref, bound))
        if e == "dgelu_bands":
            nb = _cdiv(st.M, 64)
            stored = bound + _half_ulp(ref.abs() + bound, ty["C"])
            z = torch.zeros(nb * 64 - st.M, st.N, dtype=F64)
            band = lambda t: torch.cat([t, z]).view(nb, 64, st.N).sum(1)
            out.append(("bands", band(ref), band(stored) + 64 * U * band(ref.abs())))
    elif e == "dgelu_saved":
        out.append(("C", acc * aux, None))
    elif e == "dtanh":
        out.append(("C", acc * (1.0 - aux * aux), None))
    elif e in ("rowdot", "rowdot3"):
        out.append(("C", acc, None))
        out.append(("delta", (_rne(acc, ty["C"]) * aux).view(st.M, st.N // 64, 64).sum(-1), None))
    elif e == "atomic":
        out.append(("C", side["prefill"] + run.alpha * acc, None))
    elif e == "split":
        kq = r.get("kq", r["bk"])
        out.append(("C", torch.cat([a[:, lo:hi] @ b[lo:hi] for lo, hi in _slices(st.K, run.splits, kq)]), None))
    else:
        raise KeyError(e)
    if r["api"] == "x3" and e in ("none", "bias", "resid", "resid_drop", "dtanh"):
        c32 = out[0][1].float()
        hi = c32.to(BF)
        out.append(("planes_hi", hi.double(), None))
        out.append(("planes_lo", (c32 - hi.float()).to(BF).double(), None))
    return out


# ---------------------------------------------------------------------------------------------------------------- memory
def _win(flat, rows, cols, ld, off=PAD):
    return torch.as_strided(flat, (rows, cols), (ld, 1), off)


def _operand(x, ld, dtype, lo=None, gap=0):
    """x [rows, cols] -> (flat, plane): PAD NaN | rows x ld, the columns past cols NaN | [gap NaN | the lo plane, likewise] |
    POISON_ROWS rows of NaN | PAD NaN.  The value must be exact in dtype (a plane pair: in hi + lo)."""
    rows, cols = x.shape
    plane = rows * ld + gap if lo is not None else 0
    flat = torch.full((PAD + plane + (rows + POISON_ROWS) * ld + PAD,), NAN, dtype=dtype)
    if lo is None:
        _win(flat, rows, cols, ld).copy_(x)
        assert bool((_win(flat, rows, cols, ld).double() == x).all())
    else:
        hi = x.float().to(BF)
        rest = (x.float() - hi.float()).to(BF)
        assert bool((hi.double() + rest.double() == x).all())
        _win(flat, rows, cols, ld).copy_(hi)
        _win(flat, rows, cols, ld, PAD + plane).copy_(rest)
    return flat, plane


def _geometry(st, run=None):
    """name -> (rows, cols, ld) of every buffer of a stage (A, B) or of a launch on it (the rest)"""
    r = ROUTES[st.route]
    M, N, K = st.M, st.N, st.K
    ex = (lambda k: EXTRA[k] if st.pad else 0)
    g = {}
    api = r["api"]
    if run is None:
        if api == "g0":
            g["A"] = (TABLE_ROWS, K, K + ex("a"))
        else:
            g["A"] = (K, M, M + ex("a")) if st.layout == "TN" else (M, K, K + ex("a"))
        if api == "g1":
            g["B"] = (TABLE_ROWS, N, N + ex("b"))
        else:
            g["B"] = (N, K, K + ex("b")) if st.layout == "NT" else (K, N, N + ex("b"))
        return g
    ldc = N + ex("c")
    g["C"] = (M * run.splits if run.epi == "split" else M, N, ldc)
    g["aux2"] = (M, N, ldc)
    g["aux"] = (11 if run.epi == "tanh_add" else M, N, N + ex("aux"))
    g["bands"] = (_cdiv(M, 64), N, N)
    g["delta"] = (M, max(N // 64, 1), max(N // 64, 1))
    g["planes"] = (M, N, N + ex("p"))
    return g


@functools.lru_cache(maxsize=2)
def _stage(st):
    """the operands of a stage as stored (CPU): flats A, B (+ plane distances), the gather indices, and the values"""
    r = ROUTES[st.route]
    api = r["api"]
    a, b, acc = _values(st.M, st.N, st.K, st.pattern)
    geo = _geometry(st)
    T = r["dtype"]
    d = dict(geo=geo, planeA=0, planeB=0)
    gi = _gen(st.M, st.K, "rows")
    if api == "g0":          # A = the table, row rows[m] of it is a[m]
        rows = torch.randperm(TABLE_ROWS, generator=gi)[torch.arange(st.M) % TABLE_ROWS]
        lim = 1 if st.pattern == "sixteenths" else 3
        table = _ints((TABLE_ROWS, st.K), -lim, lim, gi)
        rows[0], rows[-1] = TABLE_ROWS - 1, 0
        a = table[rows]
        acc = a @ b
        d["rows"] = rows.int()
        d["A"], _ = _operand(table, geo["A"][2], T)
    elif api == "g1":        # B = the table, row rows[k] of it is b[k]
        rows = torch.randperm(TABLE_ROWS, generator=gi)[torch.arange(st.K) % TABLE_ROWS]
        table = _ints((TABLE_ROWS, st.N), -3, 3, gi)
        rows[0], rows[-1] = TABLE_ROWS - 1, 0
        b = table[rows]
        acc = a @ b
        d["rows"] = rows.int()
        d["B"], _ = _operand(table, geo["B"][2], T)
    x3 = api == "x3"
    gap = 16 if st.pad else 0
    if "A" not in d:
        d["A"], d["planeA"] = _operand(a.t() if st.layout == "TN" else a, geo["A"][2], T, lo=True if x3 else None, gap=gap)
    if "B" not in d:
        d["B"], d["planeB"] = _operand(b.t() if st.layout == "NT" else b, geo["B"][2], T, lo=True if x3 else None, gap=2 * gap)
    d["v"] = (a, b, acc)
    return d


def _launch_buffers(st, run, side):
    """the buffers of one launch besides A and B (CPU): name -> flat, and name -> [(output, rows, cols, ld, offset)] of the windows
    the launch may write.  Outputs hold the sentinel, the epilogue's operands NaN outside their extent."""
    geo = _geometry(st, run)
    ty = _types(st, run)
    e = run.epi
    flats, wins = {}, {}

    def output(name, dtype, planes=False):
        rows, cols, ld = geo[name]
        plane = rows * ld + (16 if st.pad else 0) if planes else 0
        flats[name] = torch.full((PAD + plane + (rows + TAIL) * ld + PAD,), SENT, dtype=dtype)
        wins[name] = [(name, rows, cols, ld, PAD)] if not planes else [("planes_hi", rows, cols, ld, PAD), ("planes_lo", rows, cols, ld, PAD + plane)]
        return plane

    output("C", ty["C"])
    if e == "atomic":
        _win(flats["C"], *geo["C"]).copy_(side["prefill"])
    if e in ("gelu", "gelu_grad"):
        output("aux2", ty["aux2"])
    if e == "dgelu_bands":
        output("bands", F32)
    if e in ("rowdot", "rowdot3"):
        output("delta", F32)
    plane_out = 0
    if ROUTES[st.route]["api"] == "x3" and e in ("none", "bias", "resid", "resid_drop", "dtanh"):
        plane_out = output("planes", BF, planes=True)
    if "bias" in side:
        flats["bias"] = torch.full((PAD + st.N + PAD,), NAN, dtype=F32)
        flats["bias"][PAD:PAD + st.N] = side["bias"].float()
    if "aux" in side:
        flats["aux"], _ = _operand(side["aux_table"] if e == "tanh_add" else side["aux"], geo["aux"][2], ty["T"])
    return flats, wins, geo, plane_out


# ---------------------------------------------------------------------------------------------------------------- verdict
def _where_from(st, v, m, n, got):
    """coded pattern: which (k, n') of B hold the value found at C[m, n]"""
    b = v[1]
    hits = (b == got).nonzero()[:4].tolist()
    return "C[%d, %d] should be B[%d, %d] = %g, found %g = B at (k, n) %s" % (m, n, m % st.K, n, float(b[m % st.K, n]), got, hits or "nowhere")


def _verify(name, st, run, v, side, after, wins):
    """failures (strings) and the worst err / allowed of the bounded outputs of one launch.  after: name -> flat (CPU) after the run"""
    fails, margin = [], {}
    expect = {o: (ref, bound) for o, ref, bound in _expect(st, run, v, side)}
    for fname, wl in wins.items():
        flat = after[fname]
        clean = flat.clone()
        for oname, rows, cols, ld, off in wl:
            ref, bound = expect[oname]
            got = _win(flat, rows, cols, ld, off).double()
            assert ref.shape == got.shape, (name, oname, ref.shape, got.shape)
            if not bool(torch.isfinite(got).all()):
                i = tuple((~torch.isfinite(got)).nonzero()[0].tolist())
                fails.append("%s %s: %d non-finite elements, first at %s" % (name, oname, int((~torch.isfinite(got)).sum()), i))
            elif bound is None:
                assert bool((ref.float().double() == ref).all()), (name, oname, "the exact reference must be an fp32 number")
                want = _rne(ref, flat.dtype)
                bad = got != want
                if bool(bad.any()):
                    i = tuple(bad.nonzero()[0].tolist())
                    msg = "%s %s: %d/%d elements differ from the exact result, first at %s: got %.9g, exact %.9g (stored as %.9g)" % (
                        name, oname, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(want[i]))
                    if st.pattern == "coded" and oname == "C" and run.epi in ("none", "split"):
                        msg += "; " + _where_from(st, v, i[0] % st.M, i[1], float(got[i]))
                    fails.append(msg)
            else:
                allowed = bound + _half_ulp(ref.abs() + bound, flat.dtype)
                err = (got - ref).abs()
                ratio = torch.where(err == 0, torch.zeros_like(err), err / allowed).nan_to_num(nan=float("inf"))
                w = float(ratio.max())
                margin["%s:%s%s" % (oname, run.epi, " f32" if flat.dtype == F32 and ROUTES[st.route]["dtype"] == BF else "")] = w
                if w > 1.0:
                    i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
                    fails.append("%s %s: %d/%d outside the bound, worst at %s: got %.9g, ref %.9g, allowed %.3g (err/allowed %.3g)" % (
                        name, oname, int((ratio > 1).sum()), ratio.numel(), i, float(got[i]), float(ref[i]), float(allowed[i]), w))
            _win(clean, rows, cols, ld, off).fill_(SENT)
        bad = clean != SENT
        if bool(bad.any()):
            o = int(bad.nonzero()[0])
            _, rows, cols, ld, off = wl[0]
            fails.append("%s %s: %d elements outside the output were written, first at offset %d = row %d, column %d of the window (ld %d): %.9g" % (
                name, fname, int(bad.sum()), o - off, (o - off) // ld, (o - off) % ld, ld, float(flat[o])))
    return fails, margin


def _label(st, run):
    return "%s %s %dx%dx%d %s %s %s%s%s" % (st.route, st.layout, st.M, st.N, st.K, st.pattern, "padded" if st.pad else "packed", run.epi,
                                           " f32" if run.f32 else "", " splits=%d alpha=%g" % (run.splits, run.alpha) if run.splits > 1 or run.alpha != 1 else "")


# =====================================================================================================================
# 3. the checker checked, without a GPU
# =====================================================================================================================
def _model(st, run, sd, side, defect=None):
    """A tiled product restated on the CPU from the operands AS STORED (through their leading dimensions): fp32 accumulation over K
    tiles inside each K split, the epilogue in fp32 (a transcendental: the float64 function rounded once to fp32), a store through the
    output type.  defect plants one of the mistakes of test_planted_defects_are_rejected.  -> name -> flat, windows"""
    r = ROUTES[st.route]
    api, bk = r["api"], r["bk"]
    tm = r["tile"][0]
    M, N, K = st.M, st.N, st.K
    geo = sd["geo"]
    flats, wins, lgeo, _ = _launch_buffers(st, run, side)

    def load(name, plane):
        rows, cols, ld = geo[name]
        x = _win(sd[name], rows, cols, ld).float()
        return x + _win(sd[name], rows, cols, ld, PAD + plane).float() if api == "x3" else x

    A, B = load("A", sd["planeA"]), load("B", sd["planeB"])
    if api == "g0":
        A = A[sd["rows"].long()]
    if api == "g1":
        B = B[sd["rows"].long()]
    a32 = A.t() if st.layout == "TN" else A
    b32 = B.t() if st.layout == "NT" else B
    e = run.epi
    kq = r.get("kq", bk)
    if e in ("split", "atomic"):
        sl = _slices(K, run.splits, kq)
    else:
        sl = [(0, K)]
    parts = []
    for si, (lo, hi) in enumerate(sl):
        acc = torch.zeros(M, N, dtype=F32)
        for ti, k0 in enumerate(range(lo, hi, bk)):
            k1 = min(k0 + bk, hi)
            t = a32[:, k0:k1] @ b32[k0:k1]
            if defect == "tile-twice" and si == 0 and ti == 0:         # one K tile taken twice in one wave tile (64 x 64)
                t[:64, :64] *= 2.0
            if defect == "last-chunk" and k1 == K and M % tm:           # the last 8-element chunk dropped in the last, ragged row tile
                m0 = M // tm * tm
                t[m0:] -= a32[m0:, K - r["ch"]:K] @ b32[K - r["ch"]:K]
            acc += t
        parts.append(acc)
    ty = _types(st, run)
    f64 = lambda fn, x: F64_FORMS[fn](x.double()).float()
    C = lgeo["C"]
    if e == "split":
        for s, acc in enumerate(parts):
            if defect == "slab-unwritten" and sl[s][0] == sl[s][1]:      # a slab past the end of K left as it was
                continue
            _win(flats["C"], M, N, C[2], PAD + s * M * C[2]).copy_(acc)
        return flats, wins
    if e == "atomic":
        out = _win(flats["C"], *C)
        for acc in parts:
            out += torch.tensor(run.alpha, dtype=F32) * acc
        return flats, wins
    acc = parts[0]
    v = acc + _win(flats["bias"], 1, N, N)[0] if "bias" in flats else acc
    aux = None
    if "aux" in flats:
        rows, cols, ld = lgeo["aux"]
        aux = _win(flats["aux"], rows, cols, N if defect == "aux-ld" else ld).float()
        if e == "tanh_add":
            aux = aux[side["aux_rows"].long()]
    trunc = (lambda x: (x.float().view(torch.int32) & -65536).view(F32).to(BF))
    store = (lambda name, x, dtype: _win(flats[name], *lgeo[name]).copy_(trunc(x) if defect == "trunc-store" and dtype == BF else x.to(dtype)))
    if e in ("gelu", "gelu_grad"):
        store("aux2", v if e == "gelu" else f64("gelu_grad", v), ty["aux2"])
        v = f64("gelu", v)
    elif e == "tanh":
        v = f64("tanh", v)
    elif e == "tanh_add":
        v = f64("tanh", v + aux)
    elif e == "resid":
        v = v + aux
    elif e == "resid_drop":
        v = v * (side["keep"].float() * 2.0) + aux
    elif e in ("dgelu", "dgelu_bands"):
        v = v * f64("gelu_grad", aux)
        if e == "dgelu_bands":
            nb = _cdiv(M, 64)
            z = torch.zeros(nb * 64 - M, N, dtype=F32)
            store("bands", torch.cat([v.to(ty["C"]).float(), z]).view(nb, 64, N).sum(1), F32)
    elif e == "dgelu_saved":
        v = v * aux
    elif e == "dtanh":
        v = v * (1.0 - aux * aux)
    elif e in ("rowdot", "rowdot3"):
        store("delta", (v.to(ty["C"]).float() * aux).view(M, N // 64, 64).sum(-1), F32)
    store("C", v, ty["C"])
    if "planes" in flats:
        hi = v.to(BF)
        (_, rows, cols, ld, o1), (_, _, _, _, o2) = wins["planes"]
        _win(flats["planes"], rows, cols, ld, o1).copy_(hi)
        _win(flats["planes"], rows, cols, ld, o2).copy_((v - hi.float()).to(BF))
    if defect == "row-past-M":                    # a row past M stored
        flats["C"][PAD + M * C[2]:PAD + M * C[2] + N] = 1.0
    if defect == "pad-column":                    # one pad column written
        assert C[2] > N
        flats["C"][PAD + N] = 1.0
    return flats, wins


def _model_case(st, run, defect=None):
    sd = _stage(st)
    side = _side(st, run)
    flats, wins = _model(st, run, sd, side, defect)
    return _verify(_label(st, run), st, run, sd["v"], side, flats, wins)


@pytest.mark.parametrize("route,layout", TESTS)
def test_tiled_model_passes_every_case(route, layout):
    """section 3: the restatement must pass every assertion of every case of the table -- what it cannot pass is a mistake of the
    table, of the reference or of a bound, not of a kernel"""
    worst, n = {}, 0
    for st, runs, kind in _cases(route, layout):
        if st.M * st.N > 2_000_000 and st.pad:          # (the largest extra shapes: the packed run covers the table's logic)
            n += len(runs)
            continue
        for run in runs:
            fails, margin = _model_case(st, run)
            assert not fails, "\n".join(fails)
            for k, w in margin.items():
                worst[k] = max(worst.get(k, 0.0), w)
            n += 1
    print("tiled model, %s %s: %d launches, worst err / allowed %s" % (route, layout, n, {k: round(w, 3) for k, w in worst.items()}))


def _find(route, layout, pred):
    for st, runs, kind in _cases(route, layout):
        for run in runs:
            if pred(st, run, kind):
                return st, run
    raise LookupError((route, layout))


# defect -> the case of the table that must reject it
DEFECTS = {
    "last-chunk": ("dma2", "NT", lambda st, run, kind: st.M % 128 and st.M > 128 and st.pattern == "ints3" and run.epi == "none"),
    "tile-twice": ("dma2", "NT", lambda st, run, kind: st.K > 64 and st.pattern == "ints3" and run.epi == "none"),
    "row-past-M": ("dma2", "NT", lambda st, run, kind: run.epi == "none"),
    "pad-column": ("dma2", "NT", lambda st, run, kind: st.pad and run.epi == "none"),
    "trunc-store": ("dma2", "NT", lambda st, run, kind: st.pattern == "ties" and st.K >= 64 and st.M >= 64 and run.epi == "none" and not run.f32),
    "aux-ld": ("dma2", "NT", lambda st, run, kind: st.pad and st.M > 1 and run.epi == "resid"),
    "slab-unwritten": ("occ4", "TN", lambda st, run, kind: run.epi == "split" and _cdiv(st.K, _kper(st.K, run.splits, 64)) < run.splits),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_are_rejected(defect):
    """section 3: the model with one defect planted must fail on a case of the table, and without it pass the same case"""
    route, layout, pred = DEFECTS[defect]
    st, run = _find(route, layout, pred)
    clean, _ = _model_case(st, run)
    assert not clean, "the model without a defect must pass: " + "\n".join(clean)
    fails, _ = _model_case(st, run, defect)
    print("defect %s on %s:" % (defect, _label(st, run)), fails)
    assert fails, "the case does not reject the defect " + defect


def test_helpers_close_accepts_a_dropped_chunk_and_barely_sees_a_doubled_tile():
    """Why this file exists: at the shapes and with the inputs of tests/test_ops_gpu.py (test_gemm_persistent_pipeline_matches_plain's
    bf16 NT product, 4741 x 2120 x 4744, rnd seeds 11 / 12, checked with close(got, ref, bf16, K)), a product that drops the last
    8-element chunk of K in the last, ragged row tile (rows 4736 .. 4740) is ACCEPTED.  One 64-deep K tile taken twice in one
    64 x 64 wave tile is not accepted there -- K would have to be above 11000 for that -- but only just: close's allowance
    (16.4 absolute) is two standard deviations of the defect's error, so 149 of the wave tile's 4096 elements are outside it
    (3.6 %: asserted below 5 %) and the other 96 % of the damaged elements pass.  The exact test of this file rejects both on
    every element they touch that changes (test_planted_defects_are_rejected)."""
    M, N, K = 4741, 2120, 4744
    a = rnd(M, K, dtype=BF, seed=11).float()
    b = rnd(K, N, dtype=BF, seed=12).float()
    ref = a @ b
    got = ref.clone()
    m0 = M // 128 * 128
    got[m0:] -= a[m0:, K - 8:] @ b[K - 8:]
    close(got, ref, BF, K, "last chunk dropped in the last row tile")
    assert float((got - ref).abs().max()) > 1.0          # (the defect is there, and it is not small: whole products are missing)
    got = ref.clone()
    got[:64, :64] += a[:64, :64] @ b[:64, :64]
    atol, rtol = tol(BF, K)
    bad = (got - ref).abs() > atol * float(ref.abs().max()) + rtol * ref.abs()
    print("one K tile twice in one wave tile: close flags %d of the 4096 damaged elements" % int(bad.sum()))
    assert 0 < int(bad.sum()) < 0.05 * 4096 and int((got != ref).sum()) > 0.99 * 4096


def test_table_is_sound():
    """the table's own promises: every route has every layout it lists; every `ties` group holds results exactly half-way between two
    bf16 values (where round-to-nearest-even, truncation and round-half-away all differ); on `ones` data |acc| <= 256, so the stored
    bf16 value is the accumulator and ROWDOT's two possible definitions agree; the coded pattern reproduces B's rows; the split
    counts are the three kinds asked for; every value of a split-precision operand is the exact sum of its planes (asserted where
    they are staged)"""
    for route, layout in TESTS:
        ties = 0
        for st, runs, kind in _cases(route, layout):
            if st.pad or st.M * st.N > 2_000_000:
                continue
            a, b, acc = _values(st.M, st.N, st.K, st.pattern)
            if st.pattern == "ties":
                c = acc.float()
                ties += int(((c.view(torch.int32) & 0xFFFF) == 0x8000).sum())      # the 16 bits a bf16 drops: exactly one half
            if st.pattern == "ones" and st.K <= 256:
                assert float(acc.abs().max()) <= 256 and bool((_rne(acc, BF) == acc).all())
            if st.pattern == "coded":
                assert bool((acc == b[torch.arange(st.M) % st.K]).all())
        if any(st.pattern == "ties" for st, _, _ in _cases(route, layout)):
            assert ties > 0, (route, layout)
    assert _split_counts(328, 64) == [1, 2, 4] and _split_counts(8, 64) == [1, 2]
    assert _slices(328, 2, 64) == [(0, 192), (192, 328)] and _slices(328, 4, 64)[-1] == (328, 328)
    assert _keep_mask(DROP_SEED, 9, 8).mean() not in (0.0, 1.0)


def test_transcendental_yardsticks():
    """section 2's measured term: float32 tanh, gelu_new and gelu_new' (the forms of common.h's fp32 branch) on the CPU against
    float64 over every multiple of 1 / 16 up to +-ARG_MAX, the arguments the table produces.  The figures printed are the source of
    TANH_YARD, GELU_YARD and GELU_GRAD_YARD; the assertion is against the allowance the kernels get.  The derived bounds of the fast
    forms are checked for their size only: positive everywhere, below 2^-17 up to |x| = 4."""
    x = torch.arange(-int(ARG_MAX) * 16, int(ARG_MAX) * 16 + 1, dtype=F64) / 16.0
    got = _f32_forms(x.float())
    for fn, scale in (("tanh", torch.ones_like(x)), ("gelu", x.abs()), ("gelu_grad", 1.0 + x * x)):
        err = (got[fn].double() - F64_FORMS[fn](x)).abs()
        rel = torch.where(scale > 0, err / scale, err)
        yard = dict(tanh=TANH_YARD, gelu=GELU_YARD, gelu_grad=GELU_GRAD_YARD)[fn]
        print("float32 %s against float64: largest error / scale %.3e (yardstick %.3e, allowed %.3e)" % (fn, float(rel.max()), yard, LIBM_FACTOR * yard))
        assert float(rel.max()) <= LIBM_FACTOR * yard, (fn, float(rel.max()))
        assert bool((err <= _libm_err(fn, x)).all())
    for fn in ("tanh", "gelu", "gelu_grad"):
        small = x.abs() <= 4.0            # (gelu_new' at large x: the fp32 rounding of s, three ulp, is multiplied by x q ~ x^3 / 4)
        assert bool((FAST_ERR[fn](x) > 0).all()) and bool((FAST_ERR[fn](x)[small] < 2.0 ** -17).all()), fn


def test_case_counts():
    """the docstring's figures"""
    counts = {"%s %s" % (route, layout): sum(len(runs) for _, runs, _ in _cases(route, layout)) for route, layout in TESTS}
    total = sum(counts.values())
    print("launches per (route, layout):", counts, "total", total, "refusals", len(REFUSALS))
    assert len(TESTS) == 31 and total == 6420 and len(REFUSALS) == 16, (len(TESTS), total, len(REFUSALS))


# =====================================================================================================================
# 4. the kernel cases
# =====================================================================================================================
EPI_CODE = dict(none=H.EPI_NONE, bias=H.EPI_NONE, bias1=H.EPI_NONE, gelu=H.EPI_GELU, gelu_grad=H.EPI_GELU, tanh=H.EPI_TANH,
                resid=H.EPI_RESID, resid_drop=H.EPI_RESID, dgelu=H.EPI_DGELU, dgelu_bands=H.EPI_DGELU, dgelu_saved=H.EPI_DGELU,
                dtanh=H.EPI_DTANH, rowdot=H.EPI_ROWDOT, rowdot3=H.EPI_ROWDOT, atomic=H.EPI_ATOMIC, split=H.EPI_SPLIT,
                tanh_add=H.EPI_TANH_ADD)


def _launch(st, run, sd, dev, geo, lgeo, plane_out, side):
    """one launch on the device buffers dev (name -> flat)"""
    r = ROUTES[st.route]
    api = r["api"]
    M, N, K = st.M, st.N, st.K
    e = run.epi
    p = lambda name: dev[name][PAD:] if name in dev else None
    aux2 = p("aux2") if "aux2" in dev else p("bands") if "bands" in dev else p("delta")
    flags = r["flags"] | (H.GEMM_GELU_GRAD if e in ("gelu_grad", "dgelu_saved") else 0)
    if st.route.startswith("p8") and e.startswith("dgelu"):
        flags |= H.GEMM_P8          # (the dGELU product takes the eight-phase kernel only with the flag; the tile rule is the same)
    drop = dict(drop_p=0.5, drop_seed=DROP_SEED) if e == "resid_drop" else {}
    lda, ldb, ldc = geo["A"][2], geo["B"][2], lgeo["C"][2]
    ldaux = lgeo["aux"][2] if "aux" in dev else 0
    if api == "gemm":
        H.gemm(p("A"), p("B"), p("C"), M, N, K, transA=st.layout == "TN", transB=st.layout == "NT", lda=lda, ldb=ldb, ldc=ldc,
               bias=p("bias"), epi=EPI_CODE[e], aux=p("aux"), ldaux=ldaux, aux2=aux2, out_f32=run.f32, alpha=run.alpha,
               splits=run.splits, flags=flags, **drop)
    elif api == "x3":
        planes = H.Planes(p("planes"), M, N, lgeo["planes"][2], plane_out) if "planes" in dev else None
        H.gemm_x3(H.Planes(p("A"), M, K, lda, sd["planeA"]), H.Planes(p("B"), N, K, ldb, sd["planeB"]), p("C"), M, N, K, planes=planes,
                  ldc=ldc, bias=p("bias"), epi=EPI_CODE[e], aux=p("aux"), ldaux=ldaux, aux2=aux2, flags=flags, **drop)
    elif api == "g0":
        H.gemm_gather(0, p("A"), p("B"), p("C"), M, N, K, dev["rows"], TABLE_ROWS, lda=lda, ldb=ldb, ldc=ldc, bias=p("bias"),
                      epi=EPI_CODE[e], aux=p("aux"), ldaux=ldaux, aux_rows=dev.get("aux_rows"))
    else:
        H.gemm_gather(1, p("A"), p("B"), p("C"), M, N, K, dev["rows"], TABLE_ROWS, lda=lda, ldb=ldb, ldc=ldc, epi=H.EPI_SPLIT,
                      splits=run.splits)


def _records(st, run):
    """workgroup records the route's kernel leaves in the trace buffer"""
    r = ROUTES[st.route]
    if not r.get("trace"):
        return 0
    tm, tn = r["trace"]
    kq = r.get("kq", r["bk"])
    s = run.splits if run.epi == "split" else _cdiv(st.K, _kper(st.K, run.splits, kq))
    return _cdiv(st.M, tm) * _cdiv(st.N, tn) * s


_mask_checked = set()


def _check_mask_on_device(M, N):
    """the CPU restatement of the dropout hash against hip.dropout_apply (same seed, same packed [M, N])"""
    if (M, N) in _mask_checked:
        return
    ones = torch.ones(M * N, device=DEV, dtype=F32)
    y = torch.empty_like(ones)
    hip.dropout_apply(ones, y, M * N, 0.5, DROP_SEED)
    assert torch.equal(y.cpu().view(M, N).double(), _keep_mask(DROP_SEED, M, N) * 2.0), "dropout mask of %dx%d" % (M, N)
    _mask_checked.add((M, N))


@gpu
@pytest.mark.parametrize("route,layout", TESTS)
def test_gemm_route(route, layout):
    """section 4: every launch of the (route, layout) on the device: exact results, bounds, sentinels, NaN poison, the route"""
    r = ROUTES[route]
    worst, n, traced = {}, 0, 0
    fails = []
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        for st, runs, kind in _cases(route, layout):
            sd = _stage(st)
            geo = sd["geo"]
            ops = {k: sd[k].to(DEV) for k in ("A", "B", "rows") if k in sd}
            budget = r.get("extra_budget", 0) if kind.startswith("extra") else r.get("budget", 0)
            hip.gemm_cu_budget(budget)
            for ri, run in enumerate(runs):
                side = _side(st, run)
                if run.epi == "resid_drop":
                    _check_mask_on_device(st.M, st.N)
                flats, wins, lgeo, plane_out = _launch_buffers(st, run, side)
                dev = dict(ops)
                dev.update({k: f.to(DEV) for k, f in flats.items()})
                if "aux_rows" in side:
                    dev["aux_rows"] = side["aux_rows"].to(DEV)
                trace = ri == 0 and not st.pad and r["api"] in ("gemm", "x3")
                if trace:
                    buf = torch.zeros(2048, 6, device=DEV, dtype=torch.int64)
                    hip.gemm_trace(buf)
                try:
                    _launch(st, run, sd, dev, geo, lgeo, plane_out, side)
                    torch.cuda.synchronize()
                finally:
                    if trace:
                        hip.gemm_trace(None)
                if trace and (cus == 256 or not (r.get("budget") or kind.startswith("extra"))):
                    got = int((buf[:, 3] != 0).sum())
                    want = _records(st, run)
                    if got != want:
                        fails.append("%s: %d workgroup records in the trace buffer, the route writes %d" % (_label(st, run), got, want))
                    traced += 1
                after = {k: dev[k].cpu() for k in flats}
                f, margin = _verify(_label(st, run), st, run, sd["v"], side, after, wins)
                fails += f
                for k, w in margin.items():
                    worst[k] = max(worst.get(k, 0.0), w)
                n += 1
                assert len(fails) < 12, "\n".join(fails)
    finally:
        hip.gemm_cu_budget(0)
        hip.gemm_trace(None)
    print("%s %s: %d launches, %d with the route confirmed by the trace, worst err / allowed %s" % (
        route, layout, n, traced, {k: round(w, 3) for k, w in worst.items()}))
    assert not fails, "\n".join(fails)


def _refused(api="gemm", layout="NT", M=64, N=128, K=64, epi="none", flags=0, dtype=BF):
    z = lambda *s, dt=dtype: torch.zeros(*s, device=DEV, dtype=dt)
    up = lambda n: _cdiv(n, 8) * 8                   # (leading dimensions stay legal: the refusal meant is the extent's)
    lda, ldb = up(M if layout == "TN" else K), up(K if layout == "NT" else N)
    A = z(K, lda) if layout == "TN" else z(M, lda)
    B = z(N, ldb) if layout == "NT" else z(K, ldb)
    Cb = z(4, M, N, dt=F32)
    rows = torch.zeros(max(M, K), device=DEV, dtype=torch.int32)
    if api == "x3":
        hip.gemm_x3(H.Planes(z(2, M, K), M, K), H.Planes(z(2, N, K), N, K), Cb, M, N, K)
    elif api == "g0":
        hip.gemm_gather(0, A, B, z(M, N), M, N, K, rows, M, lda=lda, ldb=ldb)
    elif api == "g1":
        hip.gemm_gather(1, z(K, up(M)), z(TABLE_ROWS, N), Cb, M, N, K, rows, TABLE_ROWS, lda=up(M), ldb=N, epi=H.EPI_SPLIT)
    else:
        aux = z(M, N) if epi in ("rowdot", "dgelu_bands") else None
        aux2 = z(M, N, dt=F32) if epi in ("rowdot", "dgelu_bands") else None
        f32 = epi in ("atomic", "split")
        hip.gemm(A, B, Cb if f32 else z(M, up(N)), M, N, K, transA=layout == "TN", transB=layout == "NT", lda=lda, ldb=ldb, ldc=up(N),
                 epi=EPI_CODE[epi], aux=aux,
                 aux2=aux2, out_f32=f32, splits=2 if epi == "split" else 1, flags=flags)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("what", [x[0] for x in REFUSALS])
def test_gemm_refusals(what):
    """the (route, shape, epilogue) combinations the ABI refuses, by their error text"""
    _, kw, text = [x for x in REFUSALS if x[0] == what][0]
    with pytest.raises(RuntimeError) as err:
        _refused(**kw)
    assert text in str(err.value), str(err.value)
