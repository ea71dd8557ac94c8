"""The grouped weight-gradient kernels against a float64 product of the same integers, exactly, at their tile and K edges
(csrc/wgrad.hip, mmtg_wgrad_group: config 0 = 128x128 tiles, 1 = 256x256 eight-phase tiles, 8 = the 16-wave ring, 2 = split
precision in three passes, 6 = split precision on combined stages).

tests/test_ops_gpu.py, tests/test_wgrad_ring_gpu.py and tests/test_x3_gpu.py run these kernels on Gaussian operands at the
workload's shapes under `2e-5 max|ref|`, and accumulate onto a constant.  Here every operand is a small integer stored in bf16: every
product and every partial sum, in any order, is an fp32 integer (K max|a| max|b| < 2^24 is asserted per case), so the fp32 result
must EQUAL the float64 product A[:, :M]^T B[:, :N] whatever the tile, stage, split count or form.  Nothing in this file has a
tolerance; values are compared as numbers (-0 equals +0), memory that must not change bit for bit.

  1. the case table (data): per form a star of (M, N, K) around one ragged base shape (every M, every N, every K of the form's lists
     against the base values of the other two, plus one corner with the largest of each), the (K, splits) pairs that put every K
     slice at its edge, two groups of 8 problems (one-tile problems mixed with both `m_fast` branches; 18 tiles, so 18 and 54 work
     items: no multiple of 8); every case packed and with padded leading dimensions (lda = M + 8, ldb = N + 16, ldc = N + 4 or
     N + 12; split precision: the lo plane a NaN-filled gap behind the hi plane's NaN rows, 8 elements for A and 24 for B), in both
     write modes (overwrite onto NaN, accumulate onto start values coded by (m, n)), each launched twice;
  2. what every launch asserts (_verify): C exact on [0, M) x [0, N); bit-identical pad columns, TAIL rows behind row M and PAD
     elements in front of and behind C; bit-identical operands, NaN pad columns and POISON_ROWS NaN rows behind row K of every
     plane; bit-identical sentinels directly behind (and in front of) a workspace of exactly tiles x effective splits x TB^2
     floats and exactly tiles x waves counters; every counter zero; the second launch gives the first one's bits;
  3. the checker checked without a GPU: a CPU restatement of the grouped launch (_model: the work-item order, `tile0` / `m_fast`,
     K slices of kper, stages with the rows past the slice zeroed, fp32 accumulation, partials in split order, the m < M && n < N
     store in 8-column segments) passes _verify on every case, and is rejected by a named case with each of DEFECTS planted; the
     accumulate check of test_wgrad_group_in_kernel_reduction (constant start, 1e-6 scale) accepts the `ldc`-for-N defect;
  4. the kernel cases, one pytest test per (form, layout), the groups, the stale-partials run, the two variants behind
     MMTG_WGRAD_FENCE / MMTG_WGRAD_TOUCH in a child process each, and the entry's refusals.

Split precision: the planes are hi = bf16(v), lo = bf16(v - hi) with v == hi + lo asserted; the reference is the ABI's three-term sum
A_hi^T B_hi + A_lo^T B_hi + A_hi^T B_lo in float64.  On the `x3both` pattern (values 256 s + t, s, t in {-1, 0, 1}: 257 = 256 + 1)
A_lo^T B_lo is non-zero (test_table_is_sound), so a kernel that adds it is told from one that drops it.

Case count (a launch = one call of mmtg_wgrad_group; a case = 4 launches: overwrite twice, accumulate twice): test_case_counts
prints and pins
  config 0: 592 launches, config 1: 624, config 8: 720, config 2: 592, config 6: 592; 3120 in all; the stale-partials run adds 8 per
  form, each child process runs config 0's 560 star and split launches again, and there are 31 refusals.  Nothing is skipped on an
  MI355X.
"""
import collections
import functools
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # (section 4 runs this file as a script in a child process)
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402
import torch  # noqa: E402

from mmtg_amd import hip  # noqa: E402

gpu = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
PAD = 64                     # elements in front of and behind every buffer (16-byte aligned for every type used)
TAIL = 8                     # rows behind row M of every C (half a 16-row store band)
POISON_ROWS = 128            # NaN rows directly behind row K of every operand plane (the deepest stage: a pair of 64-k tiles)
BG0, BGMOD = 1000, 997       # what surrounds C: 1000 + (offset mod 997), so a store that lands elsewhere changes a bit
WS_SENT = 4321.0
CNT_SENT = 0x5A5A5A5A
GAP_A, GAP_B = 8, 24         # split precision, padded run: elements between the hi plane's NaN rows and the lo plane
MAXP = 8                     # problems the ABI takes per launch
REPEATS = 2                  # every (case, write mode) is launched twice


# =====================================================================================================================
# 1. the case table
# =====================================================================================================================
# Per form: the tile edge, the waves (= arrival counters) per tile, the K rows one stage of the main loop covers (config 1:
# K tiles of 64 in pairs, an even number per slice), the K quantum of a slice, plane pairs or not; the M / N and K lists, the
# base shape (M, N, K) of the star, and the (K, splits) pairs.
_MN128 = [8, 56, 64, 72, 120, 128, 136, 264]
_MN256 = _MN128 + [248, 256, 520]
_K64 = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
_KS64 = [(72, 2), (136, 3), (130, 2), (192, 3), (200, 7)]
_G128 = ((8, 8), (136, 264), (64, 72), (128, 128), (264, 136), (120, 56), (72, 8), (8, 120))
_G256 = ((8, 8), (264, 520), (64, 72), (256, 256), (520, 264), (248, 56), (72, 8), (8, 248))
FORMS = {
    0: dict(tb=128, waves=4, bk=64, kq=64, x3=False, mn=_MN128, ks=_K64, base=(72, 136, 72), splits=_KS64, group=_G128),
    1: dict(tb=256, waves=8, bk=64, kq=128, x3=False, mn=_MN256, ks=[1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257],
            base=(136, 264, 136), splits=[(136, 2), (264, 3), (384, 3), (392, 7)], group=_G256),
    8: dict(tb=256, waves=16, bk=32, kq=64, x3=False, mn=_MN256, ks=[1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193],
            base=(136, 264, 104), splits=_KS64, group=_G256),
    2: dict(tb=128, waves=4, bk=64, kq=64, x3=True, mn=_MN128, ks=_K64, base=(72, 136, 72), splits=_KS64, group=_G128),
    6: dict(tb=128, waves=4, bk=64, kq=64, x3=True, mn=_MN128, ks=_K64, base=(72, 136, 72), splits=_KS64, group=_G128),
}
CONFIGS = list(FORMS)
TESTS = [(c, pad) for c in CONFIGS for pad in (False, True)]

# shapes: ((M, N), ...) of the problems of the launch; kind: "m" / "n" / "k" / "corner" (the star), "split", "group"
Case = collections.namedtuple("Case", "config shapes K splits pattern pad kind")


def _cdiv(a, b):
    return -(-a // b)


def _split_rule(K, splits, kq):
    """(kper, effective split count) as the entry computes them: no K slice is empty"""
    kper = _cdiv(_cdiv(K, splits), kq) * kq
    return kper, _cdiv(K, kper)


def _tiles(shapes, tb):
    return sum(_cdiv(M, tb) * _cdiv(N, tb) for M, N in shapes)


def _star(config):
    f = FORMS[config]
    M0, N0, K0 = f["base"]
    out = [(M, N0, K0, "m") for M in f["mn"]] + [(M0, N, K0, "n") for N in f["mn"]] + [(M0, N0, K, "k") for K in f["ks"]]
    out.append((f["mn"][-1], f["mn"][-1], f["ks"][-1], "corner"))
    seen, uniq = set(), []
    for s in out:
        if s[:3] not in seen:
            seen.add(s[:3])
            uniq.append(s)
    return uniq


def _patterns(config, i):
    """the two value patterns of the i-th shape of a list"""
    if FORMS[config]["x3"]:
        return [("x3a", "x3b")[i % 2], "x3both"]
    return ["ints3", ("coded", "ties15")[i % 2]]


@functools.lru_cache(maxsize=None)
def _cases(config, pad, kinds=("star", "split", "group")):
    f = FORMS[config]
    M0, N0, K0 = f["base"]
    out = []
    if "star" in kinds:
        for i, (M, N, K, kind) in enumerate(_star(config)):
            out += [Case(config, ((M, N),), K, 1, p, pad, kind) for p in _patterns(config, i)]
    if "split" in kinds:
        for i, (K, s) in enumerate(f["splits"]):
            out += [Case(config, ((M0, N0),), K, s, p, pad, "split") for p in _patterns(config, i)]
    if "group" in kinds:
        Ks, s = f["splits"][1]                       # (136, 3) / (264, 3): three slices, the last one ragged
        for K, splits in ((K0, 1), (Ks, s)):
            out += [Case(config, f["group"], K, splits, p, pad, "group") for p in ("coded", "x3both" if f["x3"] else "ints3")]
    return out


# ---------------------------------------------------------------------------------------------------------------- values
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _planes(v):
    """the project's rule: hi = bf16(v), lo = bf16(v - hi); the pair must hold v exactly"""
    hi = v.float().to(BF)
    lo = (v.float() - hi.float()).to(BF)
    assert bool((hi.double() + lo.double() == v).all())
    return hi.double(), lo.double()


@functools.lru_cache(maxsize=16)
def _values(M, N, K, pattern, pidx, x3):
    """A [K, M], B [K, N] as stored (float64 planes: a_hi, a_lo, b_hi, b_lo; the lo planes None without x3) and the reference:
    A^T B, for plane pairs the ABI's three-term sum; lolo = A_lo^T B_lo, which the ABI drops"""
    g = _gen(M, N, K, pattern, pidx)
    if pattern == "ints3":
        a, b = _ints((K, M), -3, 3, g), _ints((K, N), -3, 3, g)
    elif pattern == "ties15":
        a, b = _ints((K, M), -15, 15, g), _ints((K, N), -15, 15, g)
    elif pattern == "coded":                    # A selects: C[m, :] = B[m mod K, :], and B's values say where they come from
        a = torch.zeros(K, M, dtype=F64)
        a[torch.arange(M) % K, torch.arange(M)] = 1.0
        b = ((torch.arange(K)[:, None] * N + torch.arange(N)[None, :] + 37 * pidx) % 251 - 125).double()
    elif pattern in ("x3a", "x3b"):             # one operand needs both planes (up to 4095), the other has an empty lo plane
        big, small = (-4095, 4095), (-3, 3)
        ra, rb = (big, small) if pattern == "x3a" else (small, big)
        a, b = _ints((K, M), ra[0], ra[1], g), _ints((K, N), rb[0], rb[1], g)
    elif pattern == "x3both":                   # both operands need their lo plane: 257 = 256 + 1, -257 = -256 - 1
        a = 256.0 * _ints((K, M), -1, 1, g) + _ints((K, M), -1, 1, g)
        b = 256.0 * _ints((K, N), -1, 1, g) + _ints((K, N), -1, 1, g)
    elif pattern == "randn":                    # (test_old_accumulate_check_accepts_ldc_for_n only: not exact, not in the table)
        a, b = torch.randn(K, M, generator=g).to(BF).double(), torch.randn(K, N, generator=g).to(BF).double()
    else:
        raise KeyError(pattern)
    if x3:
        (ah, al), (bh, bl) = _planes(a), _planes(b)
        amax = float(ah.abs().max() + al.abs().max())
        bmax = float(bh.abs().max() + bl.abs().max())
        ref = ah.t() @ bh + al.t() @ bh + ah.t() @ bl
        lolo = al.t() @ bl
    else:
        assert bool((a.to(BF).double() == a).all() and (b.to(BF).double() == b).all())
        ah, al, bh, bl = a, None, b, None
        amax, bmax = float(a.abs().max()), float(b.abs().max())
        ref, lolo = a.t() @ b, None
    # every partial sum of every pass, in any order, is bounded by K max|a| max|b|: below 2^24 it is an fp32 integer
    assert pattern == "randn" or K * amax * bmax < 2 ** 24, (M, N, K, pattern)
    return dict(ah=ah, al=al, bh=bh, bl=bl, ref=ref, lolo=lolo)


def _start(M, N, pidx):
    """accumulate: start values that differ per element, small integers coded by (m, n) and the problem"""
    return ((torch.arange(M)[:, None] * 7 + torch.arange(N)[None, :] * 13 + 5 * pidx) % 61 - 30).double()


# ---------------------------------------------------------------------------------------------------------------- memory
def _win(flat, rows, cols, ld, off):
    return torch.as_strided(flat, (rows, cols), (ld, 1), off)


def _operand(hi, lo, ld, gap, far):
    """-> (flat bf16, plane distance in elements).  PAD NaN | K rows x ld, the columns past the extent NaN | POISON_ROWS rows of
    NaN | PAD NaN; a plane pair holds the lo plane `plane` elements behind the hi plane: packed (far = False) directly behind
    row K of the hi plane (the ABI's default, plane = K ld), far behind the hi plane's NaN rows and `gap` more NaN elements."""
    K, cols = hi.shape
    plane = 0
    if lo is not None:
        plane = (K + POISON_ROWS) * ld + gap if far else K * ld
    flat = torch.full((PAD + plane + (K + POISON_ROWS) * ld + PAD,), NAN, dtype=BF)
    _win(flat, K, cols, ld, PAD).copy_(hi)
    if lo is not None:
        _win(flat, K, cols, ld, PAD + plane).copy_(lo)
    return flat, plane


def _geometry(case, pi):
    M, N = case.shapes[pi]
    if not case.pad:
        return M, N, N
    return M + 8, N + 16, N + (4 if (M // 8 + pi) % 2 == 0 else 12)


@functools.lru_cache(maxsize=4)
def _stage(case):
    """the operands of a case as stored (CPU), per problem: flats A, B, plane distances, leading dimensions and the values"""
    x3 = FORMS[case.config]["x3"]
    out = []
    for pi, (M, N) in enumerate(case.shapes):
        v = _values(M, N, case.K, case.pattern, pi, x3)
        lda, ldb, ldc = _geometry(case, pi)
        A, planeA = _operand(v["ah"], v["al"], lda, GAP_A, case.pad)
        B, planeB = _operand(v["bh"], v["bl"], ldb, GAP_B, case.pad)
        out.append(dict(M=M, N=N, lda=lda, ldb=ldb, ldc=ldc, A=A, B=B, planeA=planeA, planeB=planeB, v=v))
    return out


def _c_flat(p, pi, accumulate, start="coded"):
    """C before a launch: PAD | M rows x ldc | TAIL rows x ldc | PAD, the window NaN (overwrite) or the start values (accumulate),
    everything else the background"""
    M, N, ldc = p["M"], p["N"], p["ldc"]
    n = PAD + (M + TAIL) * ldc + PAD
    if start == "ones":
        return torch.ones(n, dtype=F32)
    flat = (torch.arange(n) % BGMOD + BG0).float()
    _win(flat, M, N, ldc, PAD).copy_(_start(M, N, pi) if accumulate else torch.full((M, N), NAN))
    return flat


def _work_buffers(case):
    """workspace of exactly tiles x effective splits x TB^2 floats (NaN) and exactly tiles x waves counters (zero), each with
    PAD sentinels in front of and directly behind it in the same allocation; (None, None) where the entry needs neither"""
    f = FORMS[case.config]
    _, eff = _split_rule(case.K, case.splits, f["kq"])
    if eff == 1:
        return None, None
    tiles = _tiles(case.shapes, f["tb"])
    ws = torch.full((PAD + tiles * eff * f["tb"] ** 2 + PAD,), NAN, dtype=F32)
    ws[:PAD] = WS_SENT
    ws[-PAD:] = WS_SENT
    cnt = torch.zeros(PAD + tiles * f["waves"] + PAD, dtype=I32)
    cnt[:PAD] = CNT_SENT
    cnt[-PAD:] = CNT_SENT
    return ws, cnt


# =====================================================================================================================
# 2. what every launch asserts
# =====================================================================================================================
def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(I32)


def _label(case, accumulate):
    shape = "%dx%d" % case.shapes[0] if len(case.shapes) == 1 else "group of %d" % len(case.shapes)
    return "config %d %s K=%d splits=%d %s %s %s" % (case.config, shape, case.K, case.splits, case.pattern,
                                                      "padded" if case.pad else "packed", "accumulate" if accumulate else "overwrite")


def _verify(name, case, st, accumulate, c_before, c_after, ops_after, ws_edges, cnt_after):
    """failures (strings) of one launch.  c_before / c_after: C flats per problem (CPU); ops_after: [(A, B)] flats per problem;
    ws_edges: (front PAD, back PAD) of the workspace or None; cnt_after: the counter flat or None"""
    fails = []
    for pi, p in enumerate(st):
        M, N, ldc, v = p["M"], p["N"], p["ldc"], p["v"]
        got = _win(c_after[pi], M, N, ldc, PAD).double()
        want = v["ref"] + _start(M, N, pi) if accumulate else v["ref"]
        assert bool((want.float().double() == want).all()), (name, "the exact reference must be an fp32 number")
        tag = "%s problem %d (%dx%d, ldc %d)" % (name, pi, M, N, ldc)
        if not bool(torch.isfinite(got).all()):
            bad = ~torch.isfinite(got)
            fails.append("%s: %d non-finite elements, first at %s" % (tag, int(bad.sum()), tuple(bad.nonzero()[0].tolist())))
        else:
            bad = got != want
            if bool(bad.any()):
                i = tuple(bad.nonzero()[0].tolist())
                msg = "%s: %d/%d elements differ from the exact result, first at %s: got %.9g, exact %.9g" % (
                    tag, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i]))
                if case.pattern == "coded" and not accumulate:
                    hits = [(q, tuple(h)) for q, pq in enumerate(st) for h in (pq["v"]["bh"] == float(got[i])).nonzero()[:2].tolist()]
                    msg += "; C[%d, %d] should be B[%d, %d] of problem %d, the value found is B at (problem, (k, n)) %s" % (
                        i[0], i[1], i[0] % case.K, i[1], pi, hits[:4] or "nowhere")
                fails.append(msg)
        # bit-identical: pad columns, TAIL rows, PAD in front and behind
        a, b = _bits(c_after[pi]).clone(), _bits(c_before[pi]).clone()
        _win(a, M, N, ldc, PAD).zero_()
        _win(b, M, N, ldc, PAD).zero_()
        if not torch.equal(a, b):
            o = int((a != b).nonzero()[0]) - PAD
            fails.append("%s: %d elements outside C were written, first at offset %d = row %d, column %d: %.9g" % (
                tag, int((a != b).sum()), o, o // ldc, o % ldc, float(c_after[pi][o + PAD])))
        for nm, flat in zip("AB", ops_after[pi]):
            if not torch.equal(_bits(flat), _bits(p[nm])):
                fails.append("%s: operand %s was written" % (tag, nm))
    if ws_edges is not None:
        for where, e in zip(("in front of", "behind"), ws_edges):
            if not bool((e == WS_SENT).all()):
                fails.append("%s: %d workspace sentinels %s the workspace were written" % (name, int((e != WS_SENT).sum()), where))
        if not bool((cnt_after[:PAD] == CNT_SENT).all() and (cnt_after[-PAD:] == CNT_SENT).all()):
            fails.append("%s: counter sentinels were written" % name)
        if bool((cnt_after[PAD:-PAD] != 0).any()):
            fails.append("%s: %d counters are not zero after the launch" % (name, int((cnt_after[PAD:-PAD] != 0).sum())))
    return fails


class _Backend:
    """where a case runs: put (CPU flat -> the backend's), get (back to the CPU), launch"""
    repeats = REPEATS


def _check_case(case, be, defect=None, start="coded"):
    """both write modes of one case on backend be, each launched be.repeats times -> failures"""
    st = _stage(case)
    ops = [(be.put(p["A"]), be.put(p["B"])) for p in st]
    ws0, cnt0 = _work_buffers(case)
    ws, cnt = (None, None) if ws0 is None else (be.put(ws0), be.put(cnt0))
    fails = []
    for accumulate in (False, True):
        name = _label(case, accumulate)
        c_before = [_c_flat(p, pi, accumulate, start) for pi, p in enumerate(st)]
        first = None
        for rep in range(be.repeats):
            if rep == 0 or accumulate:
                Cs = [be.put(c) for c in c_before]
            be.launch(case, st, ops, Cs, ws, cnt, accumulate, defect)
            c_after = [be.get(c) for c in Cs]
            if rep == 0:
                edges = None if ws is None else (be.get(ws[:PAD]), be.get(ws[-PAD:]))
                fails += _verify(name, case, st, accumulate, c_before, c_after, [(be.get(a), be.get(b)) for a, b in ops], edges,
                                 None if cnt is None else be.get(cnt))
                first = c_after
            else:
                if any(not torch.equal(_bits(x), _bits(y)) for x, y in zip(first, c_after)):
                    fails.append("%s: launch %d on the same buffers gives other bits than the first" % (name, rep + 1))
                if cnt is not None and bool((be.get(cnt)[PAD:-PAD] != 0).any()):
                    fails.append("%s: counters are not zero after launch %d" % (name, rep + 1))
    return fails


# =====================================================================================================================
# 3. the checker checked, without a GPU
# =====================================================================================================================
def _xcd_item(bid, nwg):
    """wg_locate's work order: workgroup bid of nwg -> item v = split * tiles + tile (every XCD one contiguous run of v)"""
    xcd, qq, rr = bid & 7, nwg >> 3, nwg & 7
    return (xcd * (qq + 1) if xcd < rr else rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3)


def _problem_table(shapes, tb):
    """the entry's per-problem tile grid: tiles_m, tiles_n, tile0, m_fast"""
    out, tiles = [], 0
    for M, N in shapes:
        tm, tn = _cdiv(M, tb), _cdiv(N, tb)
        out.append(dict(tm=tm, tn=tn, tile0=tiles, m_fast=tn > tm))
        tiles += tm * tn
    return out, tiles


def _locate(table, tiles, v, tb, defect=None):
    """item v -> (problem, tile, split, m0, n0)"""
    split, t = divmod(v, tiles)
    pi = 0
    for i in range(1, len(table)):
        if (t > table[i]["tile0"]) if defect == "tile0" else (t >= table[i]["tile0"]):
            pi = i
    P = table[pi]
    tl = t - P["tile0"]
    if P["m_fast"]:
        m0, n0 = (tl % P["tm"]) * tb, (tl // P["tm"]) * tb
        if defect == "mfast":                          # the m-fast order with the roles of m and n transposed
            m0, n0 = n0, m0
    else:
        m0, n0 = (tl // P["tn"]) * tb, (tl % P["tn"]) * tb
    return pi, t, split, m0, n0


def _stage_tile(flat, off, ld, k0, rows, bk, c0, ncols, tb):
    """[bk, tb] fp32 of a stage: rows k0 .. k0 + rows of the operand, columns c0 .. of its extent ncols; the rest zero (requested
    out of range)"""
    out = torch.zeros(bk, tb, dtype=F32)
    cols = min(tb, ncols - c0)
    if rows > 0 and cols > 0:
        out[:rows, :cols] = _win(flat, rows, cols, ld, PAD + off + k0 * ld + c0).float()
    return out


def _model(case, st, ops, Cs, accumulate, defect=None):
    """The grouped launch restated on the CPU from the operands AS STORED (through their leading dimensions and plane distances),
    writing the C flats in place.  defect plants one of DEFECTS."""
    f = FORMS[case.config]
    tb, bk, x3 = f["tb"], f["bk"], f["x3"]
    K = case.K
    kper, eff = _split_rule(K, case.splits, f["kq"])
    table, tiles = _problem_table(case.shapes, tb)
    nwg = tiles * eff
    parts = {}
    for bid in range(nwg):
        pi, t, split, m0, n0 = _locate(table, tiles, _xcd_item(bid, nwg), tb, defect)
        p = st[pi]
        A, B = ops[pi]
        kbeg = split * kper
        klen = max(0, min(K, kbeg + kper) - kbeg)
        nst = 2 * _cdiv(klen, 128) if case.config == 1 else _cdiv(klen, bk)
        passes = [(0, 0)]
        if x3:
            pa = K * p["lda"] if defect == "packed-plane" else p["planeA"]
            passes = [(0, 0), (pa, 0), (0, p["planeB"])] + ([(pa, p["planeB"])] if defect == "lolo" else [])
        acc = torch.zeros(tb, tb, dtype=F32)
        for offa, offb in passes:
            prev = None
            for s in range(nst):
                rows = bk if defect == "ragged" else max(0, min(bk, klen - s * bk))      # rows at or past the slice end: zero
                cur = (_stage_tile(A, offa, p["lda"], kbeg + s * bk, rows, bk, m0, p["M"], tb),
                       _stage_tile(B, offb, p["ldb"], kbeg + s * bk, rows, bk, n0, p["N"], tb))
                at, bt = prev if (defect == "ring-stale" and prev is not None) else cur
                prev = cur
                acc += at.t() @ bt
        parts[(t, split)] = (pi, m0, n0, acc)
    for t in range(tiles):
        pi, m0, n0, _ = parts[(t, 0)]
        p = st[pi]
        M, N, ldc = p["M"], p["N"], p["ldc"]
        total = torch.zeros(tb, tb, dtype=F32)
        for s in range(eff - 1 if (defect == "split-dropped" and eff > 1) else eff):      # partials in split order
            total += parts[(t, s)][3]
        # the store: rows m < M, 8-column segments with n < N
        mlim = _cdiv(M, 16) * 16 if defect == "band" else M
        nlim = N + 8 if defect == "pad-column" else N
        rows, cols = min(tb, mlim - m0), min(tb, nlim - n0)
        if rows <= 0 or cols <= 0:
            continue
        assert cols % 8 == 0
        dst = _win(Cs[pi], rows, cols, ldc, PAD + m0 * ldc + n0)
        if accumulate:
            ldr = N if defect == "acc-ldc" else ldc
            dst.copy_(_win(Cs[pi], rows, cols, ldr, PAD + m0 * ldr + n0).clone() + total[:rows, :cols])
        else:
            dst.copy_(total[:rows, :cols])


class _ModelBackend(_Backend):
    repeats = 1          # (a pure function of its inputs: a second run says nothing)

    def put(self, t):
        return t.clone()

    def get(self, t):
        return t

    def launch(self, case, st, ops, Cs, ws, cnt, accumulate, defect):
        _model(case, st, ops, Cs, accumulate, defect)


@pytest.mark.parametrize("config,pad", TESTS)
def test_model_passes_every_case(config, pad):
    """section 3: the restatement must pass every assertion of every case of the table -- what it cannot pass is a mistake of the
    table or of the reference, not of a kernel"""
    be = _ModelBackend()
    n = 0
    for case in _cases(config, pad):
        fails = _check_case(case, be)
        assert not fails, "\n".join(fails)
        n += 1
    print("model, config %d %s: %d cases" % (config, "padded" if pad else "packed", n))


def _find(config, pad, pred):
    for case in _cases(config, pad):
        if pred(case):
            return case
    raise LookupError((config, pad))


# defect -> (config, padded?, the case of the table that must reject it)
DEFECTS = {
    # a ragged last stage that is not zeroed: it reads the NaN rows behind row K
    "ragged": (0, True, lambda c: c.kind == "k" and c.K == 65 and c.pattern == "ints3"),
    # a ring slot read one stage stale (stage s computed from the operands of stage s - 1)
    "ring-stale": (8, False, lambda c: c.kind == "k" and c.K == 97),
    # one split left out of the reduction
    "split-dropped": (1, False, lambda c: c.kind == "split" and c.K == 136),
    # accumulate reads its start value with ldc taken for N
    "acc-ldc": (0, True, lambda c: c.kind == "m" and c.shapes[0][0] == 8),
    # an item located one tile past a tile0 boundary
    "tile0": (8, False, lambda c: c.kind == "group" and c.pattern == "coded" and c.splits == 1),
    # the m-fast order transposed
    "mfast": (0, False, lambda c: c.kind == "group" and c.pattern == "coded" and c.splits == 3),
    # the A_lo pass reads at the packed plane distance K lda instead of the given one
    "packed-plane": (2, True, lambda c: c.kind == "k" and c.pattern == "x3a"),
    # A_lo^T B_lo added
    "lolo": (6, False, lambda c: c.kind == "m" and c.pattern == "x3both"),
    # a 16-row band stored past row M when M % 16 == 8
    "band": (8, False, lambda c: c.kind == "m" and c.shapes[0][0] == 248),
    # a store into a pad column
    "pad-column": (1, True, lambda c: c.kind == "n" and c.shapes[0][1] == 520),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_are_rejected(defect):
    """section 3: the model with one defect planted must fail on a named case of the table, and without it pass the same case"""
    config, pad, pred = DEFECTS[defect]
    case = _find(config, pad, pred)
    be = _ModelBackend()
    clean = _check_case(case, be)
    assert not clean, "the model without a defect must pass: " + "\n".join(clean)
    fails = _check_case(case, be, defect)
    print("defect %s on %s:" % (defect, _label(case, False)), fails[:3])
    assert fails, "the case does not reject the defect " + defect


def test_old_accumulate_check_accepts_ldc_for_n():
    """Why this file exists.  test_wgrad_group_in_kernel_reduction (tests/test_ops_gpu.py) checks accumulate as
    |acc - 1 - over| <= 1e-6 scale on Gaussian operands with C = ones everywhere, pad columns included.  Run on the CPU model at one
    of its shapes (128 x 128, K = 200, padded leading dimensions), that check ACCEPTS an accumulate that reads its start value with
    ldc taken for N: whatever element of C the tile reads, it reads 1.0.  (One tile, whose start values the model reads before it
    stores: with more tiles the misplaced reads can meet another tile's result, and whether they do is a matter of order.)  The
    same defect on this file's table (start values coded by (m, n)) is rejected (test_planted_defects_are_rejected)."""
    case = Case(0, ((128, 128),), 200, 1, "randn", True, "old")
    st = _stage(case)
    ops = [(p["A"], p["B"]) for p in st]
    over = [_c_flat(st[0], 0, False, "ones")]
    _model(case, st, ops, over, False)
    acc = [_c_flat(st[0], 0, True, "ones")]
    _model(case, st, ops, acc, True, "acc-ldc")
    M, N, ldc = st[0]["M"], st[0]["N"], st[0]["ldc"]
    assert ldc != N
    o, a = _win(over[0], M, N, ldc, PAD), _win(acc[0], M, N, ldc, PAD)
    scale = float(o.abs().max())
    assert float((a - 1.0 - o).abs().max()) <= 1e-6 * scale              # the old check: accepted
    assert bool((_win(acc[0], M, ldc - N, ldc, PAD + N) == 1.0).all())   # ... and its pad-column check too
    # the same model and defect with this file's start values: rejected
    named = _find(*DEFECTS["acc-ldc"])
    assert _check_case(named, _ModelBackend(), "acc-ldc") and not _check_case(named, _ModelBackend())


def test_table_is_sound():
    """the table's own promises: the coded pattern reproduces B's rows and differs between the problems of a group; x3both needs
    both lo planes and A_lo^T B_lo is non-zero on it (x3a / x3b: zero, one lo plane is empty); ties15 is there; the start values
    differ along rows and columns; every group has a work-item count that is no multiple of 8 and both m_fast branches at two or
    more tiles each way; ldc % 8 == 4 occurs; the work order is a permutation"""
    for config in CONFIGS:
        f = FORMS[config]
        tb = f["tb"]
        pats = set()
        for case in _cases(config, False):
            pats.add(case.pattern)
            for pi, (M, N) in enumerate(case.shapes):
                v = _values(M, N, case.K, case.pattern, pi, f["x3"])
                if case.pattern == "coded":
                    assert bool((v["ref"] == v["bh"][torch.arange(M) % case.K]).all())
                if case.pattern == "x3both":
                    assert bool((v["al"] != 0).any() and (v["bl"] != 0).any() and (v["lolo"] != 0).any()), (config, M, N, case.K)
                if case.pattern in ("x3a", "x3b"):
                    assert not bool((v["lolo"] != 0).any()) and bool(((v["al"] != 0).any() or (v["bl"] != 0).any()))
            if case.kind == "group":
                assert len(case.shapes) == MAXP
                table, tiles = _problem_table(case.shapes, tb)
                _, eff = _split_rule(case.K, case.splits, f["kq"])
                assert (tiles * eff) % 8 != 0, (config, tiles, eff)
                for fast in (True, False):
                    assert any(P["m_fast"] == fast and P["tm"] >= 2 and P["tn"] >= 2 for P in table)
                assert sum(P["tm"] * P["tn"] == 1 for P in table) >= 4
                if case.pattern == "coded":
                    assert float(_values(8, 8, case.K, "coded", 0, f["x3"])["bh"][0, 0]) != float(_values(8, 8, case.K, "coded", 1, f["x3"])["bh"][0, 0])
        assert pats == ({"x3a", "x3b", "x3both", "coded"} if f["x3"] else {"ints3", "coded", "ties15"}), pats
        assert any(_geometry(c, 0)[2] % 8 == 4 for c in _cases(config, True))
        assert {_geometry(c, 0)[2] - c.shapes[0][1] for c in _cases(config, True)} == {4, 12}
    s = _start(24, 24, 0)
    assert bool((s[1:] != s[:-1]).all() and (s[:, 1:] != s[:, :-1]).all()) and float(s.abs().max()) <= 30
    for nwg in (1, 2, 7, 8, 9, 18, 54, 63, 64, 65):
        assert sorted(_xcd_item(b, nwg) for b in range(nwg)) == list(range(nwg))


# (K, requested splits) -> (kper, effective splits) per K quantum
SPLIT_RULE = {
    64: {(72, 2): (64, 2), (136, 3): (64, 3), (130, 2): (128, 2), (192, 3): (64, 3), (200, 7): (64, 4)},
    128: {(136, 2): (128, 2), (264, 3): (128, 3), (384, 3): (128, 3), (392, 7): (128, 4)},
}


def test_split_rule():
    """kper = cdiv(cdiv(K, splits), KQ) KQ and the effective count cdiv(K, kper), pinned for every (K, splits) pair of the table;
    the slices the issue names: 72 -> 64 + 8, 136 -> 64 + 64 + 8, 130 -> 128 + 2, 200 at 7 splits -> 4 slices, the last one 8"""
    for config in CONFIGS:
        f = FORMS[config]
        assert set(f["splits"]) == set(SPLIT_RULE[f["kq"]])
        for (K, s), want in SPLIT_RULE[f["kq"]].items():
            kper, eff = _split_rule(K, s, f["kq"])
            assert (kper, eff) == want, (config, K, s, kper, eff)
            assert kper == _cdiv(_cdiv(K, s), f["kq"]) * f["kq"] and eff == _cdiv(K, kper) and (eff - 1) * kper < K <= eff * kper
    last = lambda K, s, kq: K - (_split_rule(K, s, kq)[1] - 1) * _split_rule(K, s, kq)[0]
    assert [last(72, 2, 64), last(136, 3, 64), last(130, 2, 64), last(192, 3, 64), last(200, 7, 64)] == [8, 8, 2, 64, 8]
    assert [last(136, 2, 128), last(264, 3, 128), last(384, 3, 128), last(392, 7, 128)] == [8, 8, 128, 8]


def test_sizes_satisfy_the_entry():
    """hip.wgrad_group_sizes at the requested split count must satisfy the entry's check for every case and config: a workspace of
    tiles x effective x TB^2 floats and tiles x waves counters.  Configs 2 and 6 size as config 0."""
    for config in CONFIGS:
        f = FORMS[config]
        for pad in (False, True):
            for case in _cases(config, pad):
                tiles, nws, ncnt = hip.wgrad_group_sizes(case.shapes, case.splits, config)
                _, eff = _split_rule(case.K, case.splits, f["kq"])
                assert tiles == _tiles(case.shapes, f["tb"])
                assert nws >= tiles * eff * f["tb"] ** 2 and ncnt >= tiles * f["waves"], (case, nws, ncnt)
                assert nws == tiles * case.splits * f["tb"] ** 2 and ncnt == tiles * f["waves"]
    assert hip.wgrad_group_sizes([(256, 256)], 1, 2) == hip.wgrad_group_sizes([(256, 256)], 1, 6) == (4, 4 * 16384, 16)
    assert hip.wgrad_group_sizes([(256, 256)], 1, 0) == (4, 4 * 16384, 16)
    assert hip.wgrad_group_sizes([(256, 256)], 1, 1) == (1, 65536, 8) and hip.wgrad_group_sizes([(256, 256)], 1, 8) == (1, 65536, 16)


def _launches(cases):
    return 2 * REPEATS * len(cases)


COUNTS = {0: 592, 1: 624, 8: 720, 2: 592, 6: 592}
CHILD_LAUNCHES = 560


def test_case_counts():
    """the docstring's figures"""
    counts = {c: sum(_launches(_cases(c, pad)) for pad in (False, True)) for c in CONFIGS}
    child = sum(_launches(_cases(0, pad, ("star", "split"))) for pad in (False, True))
    print("launches per form:", counts, "total", sum(counts.values()), "per child process", child, "refusals", len(REFUSALS))
    assert counts == COUNTS and sum(counts.values()) == 3120 and child == CHILD_LAUNCHES and len(REFUSALS) == 31, (counts, child, len(REFUSALS))


# =====================================================================================================================
# 4. the kernel cases
# =====================================================================================================================
class _DeviceBackend(_Backend):
    def put(self, t):
        return t.to(DEV)

    def get(self, t):
        return t.cpu()

    def launch(self, case, st, ops, Cs, ws, cnt, accumulate, defect):
        assert defect is None
        probs = []
        for p, (A, B), C_ in zip(st, ops, Cs):
            a, b = A[PAD:], B[PAD:]
            if FORMS[case.config]["x3"]:
                a = hip.Planes(a, case.K, p["M"], p["lda"], p["planeA"])
                b = hip.Planes(b, case.K, p["N"], p["ldb"], p["planeB"])
            probs.append((a, b, C_[PAD:], p["M"], p["N"], p["lda"], p["ldb"], p["ldc"]))
        hip.wgrad_group(probs, case.K, case.splits, None if ws is None else ws[PAD:-PAD], None if cnt is None else cnt[PAD:-PAD],
                        accumulate=accumulate, config=case.config)
        torch.cuda.synchronize()


def _kernel_cases(cases):
    be = _DeviceBackend()
    fails, n = [], 0
    for case in cases:
        fails += _check_case(case, be)
        n += _launches([case])
        assert len(fails) < 12, "\n".join(fails)
    return fails, n


@gpu
@pytest.mark.parametrize("config,pad", TESTS)
def test_wgrad_form(config, pad):
    """section 4: the star and the split cases of a (form, layout) on the device, every assertion of section 2"""
    fails, n = _kernel_cases(_cases(config, pad, ("star", "split")))
    print("config %d %s: %d launches" % (config, "padded" if pad else "packed", n))
    assert not fails, "\n".join(fails)


@gpu
@pytest.mark.parametrize("config,pad", TESTS)
def test_wgrad_groups(config, pad):
    """section 4: launches of 8 problems -- one-tile problems between both m_fast branches, 18 and 54 work items (the XCD
    remainder is 2 and 6), the coded pattern carrying the problem's index"""
    fails, n = _kernel_cases(_cases(config, pad, ("group",)))
    print("config %d %s groups: %d launches" % (config, "padded" if pad else "packed", n))
    assert not fails, "\n".join(fails)


@gpu
@pytest.mark.parametrize("config", CONFIGS)
def test_wgrad_stale_partials(config):
    """on ONE workspace and ONE counter buffer, two different operand sets alternate for 8 launches at splits = 3: every result
    is exactly its own product (a partial left by the launch before must never be summed)"""
    f = FORMS[config]
    K, s = f["splits"][1]
    M0, N0, _ = f["base"]
    pats = ("x3a", "x3both") if f["x3"] else ("ints3", "ties15")
    cases = [Case(config, ((M0, N0),), K, s, p, True, "split") for p in pats]
    be = _DeviceBackend()
    ws0, cnt0 = _work_buffers(cases[0])
    ws, cnt = be.put(ws0), be.put(cnt0)
    sts = [_stage(c) for c in cases]
    ops = [[(be.put(p["A"]), be.put(p["B"])) for p in st] for st in sts]
    fails = []
    for it in range(8):
        i = it % 2
        acc = bool((it // 2) % 2)
        c_before = [_c_flat(p, pi, acc) for pi, p in enumerate(sts[i])]
        Cs = [be.put(c) for c in c_before]
        be.launch(cases[i], sts[i], ops[i], Cs, ws, cnt, acc, None)
        fails += _verify("launch %d: %s" % (it, _label(cases[i], acc)), cases[i], sts[i], acc, c_before, [be.get(c) for c in Cs],
                         [(be.get(a), be.get(b)) for a, b in ops[i]], (be.get(ws[:PAD]), be.get(ws[-PAD:])), be.get(cnt))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- variants
# The switches are read once per process (static in mmtg_wgrad_group), so each gets a fresh child.  The library does not report
# which kernel a call took: the names are pinned by hand to the getenv calls of csrc/wgrad.hip (MMTG_WGRAD_FENCE: any value,
# wgrad_group_kernel<true>; MMTG_WGRAD_TOUCH=P > 0: wgrad_group_kernel<false, 3> with a lead of P K tiles).  Both are written to give
# the default build's results.  MMTG_WGRAD_ABLATE is wrong by design (timing only) and stays out.
ENV_SETTINGS = {"fence": {"MMTG_WGRAD_FENCE": "1"}, "touch": {"MMTG_WGRAD_TOUCH": "2"}}
# a child takes about 10 s (import, 560 launches of config 0); the limit is there only to end a hang
CHILD_LIMIT = 180


def _child_main(out_path):
    report = {"fails": [], "launches": 0}
    for pad in (False, True):
        fails, n = _kernel_cases(_cases(0, pad, ("star", "split")))
        report["fails"] += fails
        report["launches"] += n
    with open(out_path, "w") as fh:
        json.dump(report, fh)


@gpu
@pytest.mark.parametrize("setting", list(ENV_SETTINGS))
def test_wgrad_variants_in_a_child_process(setting, tmp_path):
    """config 0's star and split cases under the switch, in one fresh child (started, never exec'd into; never retried).  A child
    that ends by a signal or at its time limit ends the whole session: nothing more may start on a GPU that has faulted"""
    env = {k: v for k, v in os.environ.items() if k not in ("MMTG_WGRAD_FENCE", "MMTG_WGRAD_TOUCH", "MMTG_WGRAD_ABLATE")}
    env.update(ENV_SETTINGS[setting])
    out = str(tmp_path / "report.json")
    try:
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        pytest.exit("wgrad child process (%s) ran into its time limit of %d s: treated as a hang, nothing more is started" % (setting, CHILD_LIMIT), returncode=3)
    if pr.returncode < 0:
        pytest.exit("wgrad child process (%s) ended by signal %d:\n%s" % (setting, -pr.returncode, pr.stderr[-2000:]), returncode=3)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    with open(out) as fh:
        report = json.load(fh)
    print("%s: %d launches" % (setting, report["launches"]))
    assert not report["fails"], "%d failures, first 12:\n" % len(report["fails"]) + "\n".join(report["fails"][:12])
    assert report["launches"] == CHILD_LAUNCHES


# ---------------------------------------------------------------------------------------------------------------- refusals
_CFG_TEXT = "wgrad_group: config 0 (128x128 tiles)"
_DIM_TEXT = "multiples of 8, ldc of 4"
# (what, the change to a legal launch -- config 0, 72 x 136, K = 72, splits = 2, lda 80, ldb 152, ldc 140 --, the error text)
REFUSALS = [("config %d" % c, dict(config=c), _CFG_TEXT) for c in (3, 4, 5, 9, 10, 12, 16)] + [
    ("no problem", dict(n=0), "1..8 problems"),
    ("nine problems", dict(n=9), "1..8 problems"),
    ("K = 0", dict(K=0), "K and splits must be positive"),
    ("splits = 0", dict(splits=0), "K and splits must be positive"),
    ("M = 76", dict(M=76), _DIM_TEXT),
    ("N = 132", dict(N=132), _DIM_TEXT),
    ("lda = 84", dict(lda=84), _DIM_TEXT),
    ("ldb = 156", dict(ldb=156), _DIM_TEXT),
    ("lda < M", dict(lda=64), _DIM_TEXT),
    ("ldb < N", dict(ldb=128), _DIM_TEXT),
    ("ldc = N + 2", dict(ldc=138), _DIM_TEXT),
    ("ldc < N", dict(ldc=132), _DIM_TEXT),
    ("A is null", dict(null="A"), "null operand"),
    ("B is null", dict(null="B"), "null operand"),
    ("C is null", dict(null="C"), "null operand"),
    ("A 8 bytes off", dict(off="A"), "16-byte aligned"),
    ("C 8 bytes off", dict(off="C"), "16-byte aligned"),
    ("splits = 2 without a workspace", dict(ws=None), "split products need the workspace"),
    ("splits = 2 without counters", dict(cnt=None), "split products need the workspace"),
    ("workspace one float short", dict(ws=-1), "workspace needs"),
    ("counters one short", dict(cnt=-1), "workspace needs"),
    ("x3: plane distance of A no multiple of 8", dict(config=2, planeA=4), "lo plane must lie behind"),
    ("x3: lo plane of A overlaps its hi plane", dict(config=2, planeA=-8), "lo plane must lie behind"),
    ("x3 combined: lo plane of B overlaps its hi plane", dict(config=6, planeB=-8), "lo plane must lie behind"),
]


def _refused(config=0, n=1, K=72, splits=2, M=72, N=136, lda=80, ldb=152, ldc=140, null=None, off=None, ws=0, cnt=0, planeA=0, planeB=0):
    """one call of the entry with the change applied -> (the error text or None, [C changed, workspace changed, counters changed])"""
    x3 = bool(config & 2)
    case = Case(2 if x3 else 0, ((72, 136),), 72, 2, "x3both" if x3 else "ints3", True, "refusal")
    p = _stage(case)[0]
    ws0, cnt0 = _work_buffers(case)
    c0 = _c_flat(p, 0, True)
    A, B, C_, wsd, cntd = (t.to(DEV) for t in (p["A"], p["B"], c0, ws0, cnt0))
    a = None if null == "A" else A[PAD + (4 if off == "A" else 0):]
    b = None if null == "B" else B[PAD:]
    c = None if null == "C" else C_[PAD + (2 if off == "C" else 0):]
    if x3:
        # distances counted from the smallest legal one, (K - 1) ld + extent, which is a multiple of 8
        a = hip.Planes(a, K, M, lda, p["planeA"] if not planeA else (K - 1) * lda + M + planeA)
        b = hip.Planes(b, K, N, ldb, p["planeB"] if not planeB else (K - 1) * ldb + N + planeB)
    wsv = None if ws is None else wsd[PAD:wsd.numel() - PAD + ws]
    cntv = None if cnt is None else cntd[PAD:cntd.numel() - PAD + cnt]
    err = None
    try:
        hip.wgrad_group([(a, b, c, M, N, lda, ldb, ldc)] * n, K, splits, wsv, cntv, accumulate=True, config=config)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    after = [t.cpu() for t in (C_, wsd, cntd)]
    return err, [not torch.equal(_bits(x), _bits(y)) for x, y in zip((c0, ws0, cnt0), after)]


@gpu
@pytest.mark.parametrize("what", [x[0] for x in REFUSALS])
def test_wgrad_refusals(what):
    """what the entry refuses, by its error text; C, the workspace and the counters come back bit-identical"""
    _, kw, text = [x for x in REFUSALS if x[0] == what][0]
    err, changed = _refused(**kw)
    assert err is not None, "the call was accepted"
    assert text in err, err
    assert changed == [False, False, False], "a refused call changed C, the workspace or the counters: %s" % changed


@gpu
def test_wgrad_refusal_baseline_is_legal():
    """the launch the refusals are changes of is itself accepted, for bf16 and for plane pairs (so each refusal is the change's),
    and it does write C and the workspace (so `unchanged` above says something)"""
    for config in (0, 2, 6):
        err, changed = _refused(config=config)
        assert err is None and changed == [True, True, False], (config, err, changed)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "child", "usage: test_wgrad_ops_gpu.py child <report.json>"
    _child_main(sys.argv[2])
