"""The arithmetic kernels of the token step, one operator at a time, against float64 restatements (csrc/decode.hip).

The whole-model decode tests allow bf16 logits 0.15 apart and cannot say which kernel is wrong, or at which position.  Here every
case hands ONE kernel rounded inputs and compares what it wrote with the same operation in float64 torch on those inputs:

  1. the cached attention (da_body) through all four entries and their rows= forms, at every chunk edge of both element types, the
     256-flag register limit and the last slot of the 1024-entry flag table, under masks that leave the running maximum at minus
     infinity, with NaN in every cache slot the kernel must not read and in a guard band around each cache;
  2. the step's embedding kernels (type id, key flag, conditioned row: exact);
  3. the x3 fused products: the LN-fold weight preparation, the LN-fold products (modes 0 / 1) and the in-kernel split-K reduce
     (mode 2) with its tensor, TANH and embedding residuals, and the bf16 kernel's embedding residual.

No case compares a kernel with another call of the library; the one place two entries meet is the x3 attention's plane pair, which
is ALSO required to be the split of the fp32 entry's row (after both have been compared with float64).
"""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from helpers import close, planes_of, rnd  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32


def _bits(t):
    """the tensor's storage as integers: NaN compares equal to the same NaN, -0 differs from +0"""
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _split(v):
    """the (hi, lo) bf16 pair the kernels store for an fp32 value: hi = bf16(v), lo = bf16(v - hi)"""
    hi = v.bfloat16()
    return hi, (v - hi.float()).bfloat16()


def _assert_split(pl, v, name=""):
    """the plane pair is the split of the fp32 rows v: hi = bf16(v), hi + lo within 2^-17 of v (test_split_planes_reconstructs_to_2_pow_minus_17;
    lo itself may come from a fused multiply-subtract of the value's last product, so it is not pinned bit for bit)"""
    assert torch.equal(pl.t[0], v.bfloat16()), name + ": hi plane"
    assert ((pl.float() - v).abs() <= 2.0 ** -17 * v.abs()).all(), name + ": hi + lo"


def _nan_planes(rows, cols):
    return hip.Planes(torch.full((2, rows, cols), NAN, device=DEV, dtype=BF), rows, cols)


# =====================================================================================================================
# 1. cached attention
# =====================================================================================================================
B_A, NH, DH = 3, 3, 64
D_A = NH * DH
GUARD = 4096          # NaN elements before and after each cache (a multiple of 8: the cache stays 16-byte aligned)
POSITIONS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 1023]
SPLITS = [1, 3, 4, 5, 7]
FORMS = ["attn-bf16", "attn-f32", "split-bf16", "split-f32", "split-x3", "rows-bf16", "rows-f32", "rows-x3"]
SLAB_FORMS = [f for f in FORMS if not f.startswith("attn")]


def _form_dtype(form):
    return BF if form.endswith("bf16") else F32


def _guarded_cache(dtype, Tmax, pos, seed):
    """[B, nH, Tmax, 64] inside a larger NaN tensor; finite below pos (slot 0 too at pos = 0), NaN from slot pos on"""
    n = B_A * NH * Tmax * DH
    big = torch.full((GUARD + n + GUARD,), NAN, dtype=dtype)
    nfin = max(pos, 1)
    big[GUARD:GUARD + n].view(B_A, NH, Tmax, DH)[:, :, :nfin] = rnd(B_A, NH, nfin, DH, dtype=dtype, seed=seed)
    big = big.to(DEV)
    return big, big[GUARD:GUARD + n].view(B_A, NH, Tmax, DH)


def _keep_mask(pos, Tmax, mask, wide, seed):
    ld = Tmax + 24 if wide else Tmax
    k = torch.zeros(B_A, ld, dtype=torch.int32)          # columns past pos stay 0: the kernel reads none of them
    k[:, :pos + 1] = 1
    if mask == "random":                                 # about 20 %, the token's own flag included; key 5 always stays
        g = torch.Generator().manual_seed(seed)
        k[:, :pos + 1] = (torch.rand(B_A, pos + 1, generator=g) >= 0.2).int()
        k[:, 5] = 1
    elif mask == "first":                                # the whole first chunk (both of f32's first two): m_run is still -inf
        k[:, :32] = 0
    elif mask == "own":                                  # every key but the token's own
        k[:, :pos] = 0
    elif mask == "mid":                                  # a whole chunk in the middle (and one past the 256 register flags)
        k[:, 64:96] = 0
        if pos >= 288:
            k[:, 256:288] = 0
    else:
        assert mask == "none"
    return k.to(DEV)[:, :Tmax]


def _attn_call(form, qkv, slabs, splits, bias, kv, vv, keep, posd, Tmax, rows):
    """run the entry; returns the context rows as fp32 [B, D] and, for the x3 forms, the plane pair"""
    dtype = _form_dtype(form)
    if form.endswith("x3"):
        pl = _nan_planes(B_A, D_A)
        hip.decode_attn_split_x3(slabs, splits, bias, kv, vv, keep, posd, pl, B_A, NH, DH, Tmax, rows=rows)
        return pl.float(), pl
    out = torch.full((B_A, D_A), NAN, device=DEV, dtype=dtype)
    if form.startswith("attn"):
        hip.decode_attn(qkv, kv, vv, keep, posd, out, B_A, NH, DH, Tmax)
    else:
        hip.decode_attn_split(slabs, splits, bias, kv, vv, keep, posd, out, B_A, NH, DH, Tmax, rows=rows)
    return out, None


def _attn_case(form, pos, Tmax, splits=3, mask="none", wide=False, oob_rows=False):
    dtype = _form_dtype(form)
    seed = 1000 * pos + 10 * splits + len(mask)
    kbig, kv = _guarded_cache(dtype, Tmax, pos, seed + 1)
    vbig, vv = _guarded_cache(dtype, Tmax, pos, seed + 2)
    keep = _keep_mask(pos, Tmax, mask, wide, seed + 3)
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    slabs = rnd(splits, B_A, 3 * D_A, seed=seed + 4, scale=0.5).to(DEV)
    bias = rnd(3 * D_A, seed=seed + 5, scale=0.1).to(DEV)
    # q, k, v as the kernel builds them: the slabs summed in order in fp32, plus the bias, rounded to the storage type
    acc = torch.zeros(B_A, 3 * D_A, device=DEV)
    for s in range(splits):
        acc = acc + slabs[s]
    qkv = (acc + bias).to(dtype)
    rows = None
    if form.startswith("rows"):
        g = torch.Generator().manual_seed(seed + 6)
        rows = torch.randint(0, B_A, (B_A, Tmax + 8), generator=g, dtype=torch.int32)
        rows[:, pos:] = torch.arange(B_A, dtype=torch.int32)[:, None]
        if oob_rows:                                    # the kernel clamps a table entry into the batch
            rows[:, 2:pos:7] = -1
            rows[:, 3:pos:7] = B_A
        rows = rows.to(DEV)
    # ---- float64 reference: softmax(q . K / 8) over keys 0..pos under the mask, the token's own k / v in slot pos
    q, k, v = (qkv.double()[:, i * D_A:(i + 1) * D_A].view(B_A, NH, DH) for i in range(3))
    if rows is None:
        Kp, Vp = kv[:, :, :pos].double(), vv[:, :, :pos].double()
    else:                                               # gather the prefix by the (clamped) table first
        idx = rows[:, :pos].long().clamp(0, B_A - 1)
        ar = torch.arange(pos, device=DEV)
        Kp = kv.double()[idx, :, ar].permute(0, 2, 1, 3)
        Vp = vv.double()[idx, :, ar].permute(0, 2, 1, 3)
    Kall = torch.cat([Kp, k[:, :, None]], 2)
    Vall = torch.cat([Vp, v[:, :, None]], 2)
    sc = torch.einsum("bhd,bhtd->bht", q, Kall) / 8.0
    sc = sc.masked_fill(keep[:, None, :pos + 1] == 0, float("-inf"))
    ref = torch.einsum("bht,bhtd->bhd", torch.softmax(sc, -1), Vall).reshape(B_A, D_A)
    assert torch.isfinite(ref).all()
    # ---- what the caches must hold afterwards: slot pos = the rounded k / v, every other element and the guard bands untouched
    kexp, vexp = kbig.clone(), vbig.clone()
    n = B_A * NH * Tmax * DH
    kexp[GUARD:GUARD + n].view(B_A, NH, Tmax, DH)[:, :, pos] = qkv[:, D_A:2 * D_A].view(B_A, NH, DH)
    vexp[GUARD:GUARD + n].view(B_A, NH, Tmax, DH)[:, :, pos] = qkv[:, 2 * D_A:].view(B_A, NH, DH)
    k0, v0 = kbig.clone(), vbig.clone()                 # (for the x3 forms' second look below)
    name = "%s pos=%d Tmax=%d splits=%d mask=%s" % (form, pos, Tmax, splits, mask)
    out, pl = _attn_call(form, qkv, slabs, splits, bias, kv, vv, keep, posd, Tmax, rows)
    assert torch.isfinite(out.float()).all(), name + ": a slot past the prefix leaked in"
    close(out, ref, dtype, DH, name)
    assert torch.equal(_bits(kbig), _bits(kexp)), name + ": K cache"
    assert torch.equal(_bits(vbig), _bits(vexp)), name + ": V cache"
    if pl is not None:
        # the plane pair is the split of the fp32 context row: hi = bf16(out), hi + lo within 2^-17 of it.  The fp32 row is the
        # fp32 entry's (the same kernel without the plane store), itself compared with float64 here
        kb2, vb2 = k0, v0
        o32, _ = _attn_call(form.replace("x3", "f32"), qkv, slabs, splits, bias, kb2[GUARD:GUARD + n].view(B_A, NH, Tmax, DH),
                            vb2[GUARD:GUARD + n].view(B_A, NH, Tmax, DH), keep, posd, Tmax, rows)
        close(o32, ref, F32, DH, name + " (fp32 row)")
        assert torch.equal(pl.t[0], o32.bfloat16()), name + ": hi plane"
        assert ((pl.float() - o32).abs() <= 2.0 ** -17 * o32.abs()).all(), name + ": hi + lo"


def _tmax_for(pos):
    return (pos // 8 + 1) * 8          # the smallest multiple of 8 above pos (1024 at pos = 1023)


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("form", FORMS)
def test_cached_attention_at_every_chunk_edge(form, pos):
    """One, two, three and four chunks of 32 (bf16) / 16 (f32) keys, the 256 register flags, the last LDS flag slot; the slab
    counts cycle through the unrolled four and the loop behind them; every other position passes keep with a wider row stride."""
    i = POSITIONS.index(pos)
    _attn_case(form, pos, _tmax_for(pos), splits=SPLITS[i % len(SPLITS)], wide=bool(i & 1))


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("form", SLAB_FORMS)
def test_cached_attention_slab_counts(form, splits):
    _attn_case(form, 65, 72, splits=splits)


@pytest.mark.parametrize("form", FORMS)
def test_cached_attention_in_a_roomy_cache(form):
    """Tmax well above pos: the head stride is Tmax * 64, not the prefix"""
    _attn_case(form, 33, 512, wide=True)


@pytest.mark.parametrize("mask", ["random", "first", "own", "mid"])
@pytest.mark.parametrize("pos", [129, 300])
@pytest.mark.parametrize("form", FORMS)
def test_cached_attention_masks(form, pos, mask):
    """5 / 9 chunks (bf16 / f32) and 10 / 19 with flags past the 256 that travel through registers; keep is a slice of a wider
    tensor.  A masked key's value row is weighted with an exact zero, so the slots below pos hold finite values."""
    _attn_case(form, pos, _tmax_for(pos), splits=3, mask=mask, wide=True)


@pytest.mark.parametrize("form", [f for f in FORMS if f.startswith("rows")])
def test_cached_attention_clamps_the_ancestry_table(form):
    _attn_case(form, 97, 104, splits=4, mask="random", wide=True, oob_rows=True)


# =====================================================================================================================
# 2. the step's embedding kernels
# =====================================================================================================================
EB, EP, ES, EV = 5, 6, 2, 37
SENT, MSN = 6, 4                   # columns per line; max_sent_num: line 2 = MSN - 2, line 3 = MSN - 1 (the wrap to slot 1), 4 beyond
TWO = 2 * SENT                     # a segment = two lines: lyric columns 12..23 = segment S - 1, 24.. = segment S (no conditioning)
LDSEQ = 40
# prompt (0, 5); lyric i = pos - P: first column 0, interior 2, last 5, last of segment 0 (11), first of segment 1 (12),
# interior of line MSN - 2 (14) and MSN - 1 (20), last of segment S - 1 (23), first / interior / last of segment S, line 4 (24, 26, 29)
EMBED_POS = [0, 5, 6, 8, 11, 17, 18, 20, 26, 29, 30, 32, 35]


def _embed_rule(tok, pos, b, tpw_type, tpw_mask):
    """(type id, key flag) of the token at pos: the inference branch (include/mmtg_hip.h, decode_embed; model.py:296-312)"""
    if pos < EP:
        return int(tpw_type[b, pos]), int(tpw_mask[b, pos] != 0)
    i = pos - EP
    pad = tok == 0
    edge = (i + 1) % SENT in (0, 1)
    line = i // SENT
    slot = line + 1 if line < MSN - 1 else 1
    return (0 if (edge or pad) else slot), int(not pad)


def _embed_inputs():
    g = torch.Generator().manual_seed(77)
    seq = torch.randint(1, EV, (EB, LDSEQ), generator=g, dtype=torch.int64)
    seq[1, EMBED_POS] = 0                  # PAD (an interior column among them)
    seq[2, EMBED_POS] = -3                 # below 0 and at or above V: clamped for the table, not PAD for the rule
    seq[3, EMBED_POS] = EV + 4
    seq[4, 8] = EV
    tpw_type = torch.randint(0, 3, (EB, EP), generator=g, dtype=torch.int64)
    tpw_mask = torch.randint(0, 2, (EB, EP), generator=g, dtype=torch.int64)
    return seq, tpw_type, tpw_mask


def test_embed_rule_is_the_oracles_inference_branch():
    """the restatement used below against the oracle's function, over the lines the oracle's table has (0 .. max_sent_num - 1)"""
    seq, tpw_type, tpw_mask = _embed_inputs()
    n = MSN * SENT
    sh = SimpleNamespace(msl=SENT - 2, max_seq_length=(MSN - 1) * SENT)
    types, mask = O.inference_type_ids_and_mask(sh, seq[:, EP:EP + n], tpw_type, tpw_mask, per_row=True)
    for b in range(EB):
        for pos in range(EP + n):
            assert _embed_rule(int(seq[b, pos]), pos, b, tpw_type, tpw_mask) == (int(types[b, pos]), int(mask[b, pos])), (b, pos)


@pytest.mark.parametrize("E", [64, 1032])          # below one pass of the 256-thread loop; two passes in f32 (256 x 4 = 1024 a pass)
@pytest.mark.parametrize("form", ["bf16", "f32", "x3"])
def test_decode_embed(form, E):
    dtype = BF if form == "bf16" else F32
    seq, tpw_type, tpw_mask = _embed_inputs()
    table = rnd(EV, E, dtype=dtype, seed=1).to(DEV)
    c = rnd(EB, ES, E, dtype=dtype, seed=2).to(DEV)
    seqd, ttd, tmd = seq.to(DEV), tpw_type.to(DEV), tpw_mask.to(DEV)
    for pos in EMBED_POS:
        posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
        type_out = torch.full((EB,), -9, dtype=torch.int64, device=DEV)
        keep_w = torch.full((EB, LDSEQ + 8), 7, dtype=torch.int32, device=DEV)
        keep = keep_w[:, :LDSEQ]
        args = (posd, ttd, tmd, type_out, keep, EB, EP, ES, E, TWO, EV, SENT, MSN)
        tok = seqd[:, pos].clamp(0, EV - 1)
        v = table[tok].float()
        seg = (pos - EP) // TWO
        if pos >= EP and seg < ES:                    # one add in fp32, rounded once
            v = v + c[:, seg].float()
        if form == "x3":
            x = hip.Planes(torch.full((2, EB, E), 7.0, device=DEV, dtype=BF), EB, E)
            hip.decode_embed_x3(table, seqd, c, x, *args)
            hi, lo = _split(v)
            assert torch.equal(x.t[0], hi) and torch.equal(x.t[1], lo), pos
        else:
            x = torch.full((EB, E), 7.0, device=DEV, dtype=dtype)
            hip.decode_embed(table, seqd, c, x, *args)
            assert torch.equal(x, v.to(dtype)), pos
        want = [_embed_rule(int(seq[b, pos]), pos, b, tpw_type, tpw_mask) for b in range(EB)]
        assert type_out.tolist() == [w[0] for w in want], pos
        kexp = torch.full((EB, LDSEQ + 8), 7, dtype=torch.int32)
        kexp[:, pos] = torch.tensor([w[1] for w in want], dtype=torch.int32)
        assert torch.equal(keep_w.cpu(), kexp), pos      # keep is written at column pos only


@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("D", [64, 200, 768])      # below one pass, a ragged pass, the model's width
@pytest.mark.parametrize("dtype", [BF, F32])
def test_decode_embed_add(dtype, D, with_stats):
    NPOS, NTYPE, NP = 9, 4, hip.DG_NP
    g = rnd(EB, D, dtype=dtype, seed=3).to(DEV)
    wpe = rnd(NPOS, D, dtype=dtype, seed=4).to(DEV)
    wte = rnd(NTYPE, D, dtype=dtype, seed=5).to(DEV)
    ty = torch.tensor([0, 3, 1, 2, 3], dtype=torch.int64, device=DEV)
    for pos in (0, NPOS - 1):
        posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
        # h with room for a statistics block behind it in the same allocation: without `stats` nothing is written there
        buf = torch.full((EB * D + EB * NP * 2,), NAN, device=DEV, dtype=dtype)
        tail = torch.full((EB, NP, 2), NAN, device=DEV)
        h = buf[:EB * D].view(EB, D)
        hip.decode_embed_add(g, wpe, wte, ty, posd, h, EB, D, stats=tail if with_stats else None)
        want = ((g.float() + wpe[pos].float()) + wte[ty].float()).to(dtype)
        assert torch.equal(h, want), pos
        assert torch.isnan(buf[EB * D:]).all()
        if not with_stats:
            continue
        hs = h.double()
        close(tail[:, 0, 0], hs.sum(1), F32, D, "row sums")
        close(tail[:, 0, 1], (hs * hs).sum(1), F32, D, "row sums of squares")
        assert (tail[:, 1:] == 0).all()


# =====================================================================================================================
# 3. the x3 fused products
# =====================================================================================================================
U32 = 2.0 ** -24          # unit roundoff of fp32: a sum of n + 1 terms in ANY order is within n u (1 + O(u)) sum |terms| of exact


def _fold_adds(K):
    """fp32 additions on the path of one term of ln_fold_x3_kernel's row sums: a lane's 8 elements per 512-column pass in sequence,
    the add that forms the term, six butterfly steps (+ 1 of slack for the (1 + O(u)) factor)"""
    return 8 * math.ceil(K / 512) + 1 + 6 + 1


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("K", [64, 520, 768])      # below one wave pass, ragged, the model's width
@pytest.mark.parametrize("N", [5, 260])            # a ragged last workgroup of four rows
def test_ln_fold_weights_x3_against_its_definition(N, K, with_bias):
    g = torch.Generator(device=DEV).manual_seed(N + K)
    Wp = planes_of(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    w = Wp.float()                                  # the operand the kernel reconstructs: hi + lo in fp32 (exact)
    gamma = 1.0 + 0.1 * torch.randn(K, device=DEV, generator=g)
    beta = 0.1 * torch.randn(K, device=DEV, generator=g)
    bias = 0.1 * torch.randn(N, device=DEV, generator=g) if with_bias else None
    Wf = _nan_planes(N, K)
    c, bf = torch.full((N,), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
    hip.ln_fold_weights_x3(Wp, gamma, beta, bias, Wf, c, bf, N, K)
    f = gamma[None, :] * w                          # one fp32 product
    _assert_split(Wf, f, "Wf")
    stored = Wf.t[0].double() + Wf.t[1].double()
    f64 = gamma.double()[None, :] * w.double()
    assert ((stored - f64).abs() <= (2.0 ** -17 + 2.0 ** -23) * f64.abs()).all()
    # colsum = the sum of what was STORED; bias_f = bias + W beta: float64 sums, the worst-case error of the kernel's fp32 order
    n = _fold_adds(K)
    assert ((c.double() - stored.sum(1)).abs() <= n * U32 * stored.abs().sum(1)).all()
    terms = beta.double()[None, :] * w.double()
    b64 = bias.double() if with_bias else torch.zeros(N, device=DEV, dtype=torch.float64)
    assert ((bf.double() - (b64 + terms.sum(1))).abs() <= (n + 2) * U32 * (terms.abs().sum(1) + b64.abs())).all()


def test_ln_fold_x3_colsum_sums_the_stored_pair_not_the_fp32_product():
    """gamma = 1 + 2^-9 + t with 0 < t < 2^-17 on weights that are powers of two: hi = w, lo = 2^-9 w, and t -- below half an ulp
    of lo -- is dropped by the split.  Every partial sum of the stored pair is a multiple of 2^-11 below 2^12, so colsum is EXACTLY
    K (1 + 2^-9) w whatever the order; a sum of the fp32 products would carry K t on top (70 fp32 ulps at K = 768)."""
    N, K = 5, 768
    scale = torch.tensor([1.0, 2.0, 0.5, -1.0, -4.0], device=DEV)
    Wp = planes_of(scale[:, None].expand(N, K).contiguous())
    t = torch.tensor([2.0 ** -18, 2.0 ** -18 + 2.0 ** -19, 2.0 ** -18 + 2.0 ** -20], device=DEV)[torch.arange(K, device=DEV) % 3]
    gamma = (1.0 + 2.0 ** -9) + t
    assert (gamma.double() == 1.0 + 2.0 ** -9 + t.double()).all()
    beta = torch.zeros(K, device=DEV)
    Wf = _nan_planes(N, K)
    c, bf = torch.full((N,), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
    hip.ln_fold_weights_x3(Wp, gamma, beta, None, Wf, c, bf, N, K)
    assert torch.equal(Wf.t[0].float(), scale[:, None].expand(N, K))
    assert torch.equal(Wf.t[1].float(), (scale * 2.0 ** -9)[:, None].expand(N, K))
    assert torch.equal(c, scale * (K * (1.0 + 2.0 ** -9)))
    assert (bf == 0).all()


# ---- the LN-fold products (modes 0 and 1)
# The project's bound for an x3 product against float64, 4e-5 sqrt(K) rms(A) rms(W), does not transfer: the fold subtracts
# mu * colsum from the product.  Measured instead on an MI355X (docs/experiments.md, "LN-fold x3 products against float64"): on
# these very inputs the explicit path the trainer uses, mmtg_layernorm_fwd_x3 into mmtg_gemm_x3, is at most 4.71e-5 of
# sqrt(K) * rms(LN(x)) * rms(W) from the float64 reference (the largest over M x K x {plain, GELU}: M = 200, K = 64, GELU; the
# smallest 1.26e-5).  The fused form is allowed LN_FACTOR = 4 times that -- one more rounding (gamma (.) W re-split) and one
# cancellation; it measured 2.93e-5 at its worst (M = 64, K = 64, GELU), 0.62 of the explicit path's worst.
LN_REF_ERR = 4.71e-5
LN_FACTOR = 4.0


def _ln_inputs(M, K, N=100):
    g = torch.Generator(device=DEV).manual_seed(31 * M + K)
    x0 = torch.randn(M, K, device=DEV, generator=g) * 2.0 + torch.randn(M, 1, device=DEV, generator=g)      # a row offset
    x0[:, 5] *= 20.0                                                                                        # an outlier channel
    xp = planes_of(x0)
    x = xp.float().double()                    # what the product multiplies
    Wp = planes_of(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    w = Wp.float().double()
    gamma = 1.0 + 0.1 * torch.randn(K, device=DEV, generator=g)
    beta = 0.1 * torch.randn(K, device=DEV, generator=g)
    bias = 0.1 * torch.randn(N, device=DEV, generator=g)
    # the statistics partials of the rows as stored: 32-column (sum, sum of squares), fp32
    st = torch.zeros(M, hip.DG_NP, 2, device=DEV)
    st[:, :K // 32, 0] = x.view(M, K // 32, 32).sum(2).float()
    st[:, :K // 32, 1] = (x * x).view(M, K // 32, 32).sum(2).float()
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    a = (x - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
    ref = a @ w.t() + bias.double()
    scale = math.sqrt(K) * a.pow(2).mean().sqrt().item() * w.pow(2).mean().sqrt().item()
    Wf = _nan_planes(N, K)
    c, bf = torch.full((N,), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
    hip.ln_fold_weights_x3(Wp, gamma, beta, bias, Wf, c, bf, N, K)
    return SimpleNamespace(M=M, K=K, N=N, xp=xp, Wp=Wp, gamma=gamma, beta=beta, bias=bias, st=st, ref=ref, scale=scale, Wf=Wf, c=c, bf=bf,
                           x32=xp.float())


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


LN_SHAPES = [(M, K) for M in (3, 64, 200) for K in (64, 384, 768)]      # one stage, more stages than the ring is deep, the model's width


@pytest.mark.parametrize("act", ["plain", "gelu"])
@pytest.mark.parametrize("M,K", LN_SHAPES)
def test_decode_gemm_x3_ln_fold_rows_and_planes(M, K, act):
    """mode 0 at N = 100 (a ragged last column tile): float64 LN(x) W^T + b from explicit mean and variance; fp32 rows, and the
    plane-pair output = the split of those rows."""
    p = _ln_inputs(M, K)
    ref = _gelu64(p.ref) if act == "gelu" else p.ref
    epi = hip.EPI_GELU if act == "gelu" else hip.EPI_NONE
    C = torch.full((M, p.N), NAN, device=DEV)
    hip.decode_gemm_x3(0, p.xp, p.Wf, M, p.N, K, C_=C, bias=p.bf, colsum=p.c, stats_in=p.st, np_in=K // 32, act=epi)
    err = (C.double() - ref).abs().max().item()
    print("LN-fold mode 0 M=%d K=%d %s: err %.3e = %.3e of the scale %.3e" % (M, K, act, err, err / p.scale, p.scale))
    assert err <= LN_FACTOR * LN_REF_ERR * p.scale, (err, err / p.scale)
    Cp = _nan_planes(M, p.N)
    hip.decode_gemm_x3(0, p.xp, p.Wf, M, p.N, K, Cp=Cp, bias=p.bf, colsum=p.c, stats_in=p.st, np_in=K // 32, act=epi)
    _assert_split(Cp, C, "mode 0 planes")


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("M,K", LN_SHAPES)
def test_decode_gemm_x3_ln_fold_slabs(M, K, S):
    """mode 1: the slabs summed in order, plus the folded bias, against the same reference (K = 64 is one slab whatever is asked)"""
    p = _ln_inputs(M, K)
    kper = -(-(-(-K // S)) // 64) * 64
    S_eff = -(-K // kper)
    slabs = torch.full((S, M, p.N), NAN, device=DEV)
    hip.decode_gemm_x3(1, p.xp, p.Wf, M, p.N, K, C_=slabs, colsum=p.c, stats_in=p.st, np_in=K // 32, splits=S)
    assert torch.isnan(slabs[S_eff:]).all()
    got = slabs[:S_eff].double().sum(0) + p.bf.double()
    err = (got - p.ref).abs().max().item()
    print("LN-fold mode 1 M=%d K=%d S=%d: err %.3e = %.3e of the scale" % (M, K, S, err, err / p.scale))
    assert err <= LN_FACTOR * LN_REF_ERR * p.scale, (err, err / p.scale)


# ---- the in-kernel split-K reduce (mode 2)
R_SHAPES = [(64, 1), (384, 1), (384, 4), (768, 1), (768, 4), (1024, 8)]          # (K, splits asked): 384 / 4 gives three slices of 128


def _stats_check(so, rows64, N, name):
    """partials = the sums over the stored rows: 8 values per lane in sequence and two folds, so 10 fp32 additions"""
    M, npo = rows64.shape[0], N // 32
    seg = rows64.view(M, npo, 32)
    assert ((so[:, :npo, 0].double() - seg.sum(2)).abs() <= 10 * U32 * seg.abs().sum(2)).all(), name + ": sums"
    assert ((so[:, :npo, 1].double() - (seg * seg).sum(2)).abs() <= 11 * U32 * (seg * seg).sum(2)).all(), name + ": sums of squares"
    assert torch.isnan(so[:, npo:]).all(), name + ": partials past N / 32"


@pytest.mark.parametrize("kind", ["resid", "tanh", "emb"])
@pytest.mark.parametrize("N", [96, 768])
@pytest.mark.parametrize("K,S", R_SHAPES)
@pytest.mark.parametrize("M", [3, 64, 200])
def test_decode_gemm_x3_reduce(M, K, S, N, kind):
    """v = act(sum of the K slices + bias) + residual against float64, within the project's bound for a plain x3 product
    (4e-5 sqrt(K) rms(A) rms(W), test_gemm_x3_vs_float64; tanh' <= 1) plus the fp32 rounding of the residual add and the store."""
    g = torch.Generator(device=DEV).manual_seed(7 * M + K + N + S)
    Ap = planes_of(torch.randn(M, K, device=DEV, generator=g) * 0.5)
    Wp = planes_of(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    a, w = Ap.float().double(), Wp.float().double()
    bias = 0.1 * torch.randn(N, device=DEV, generator=g)
    acc = a @ w.t() + bias.double()
    kw = {}
    if kind == "emb":
        NPOS, NTYPE = 7, 4
        wpe = torch.randn(NPOS, N, device=DEV, generator=g)
        wte = torch.randn(NTYPE, N, device=DEV, generator=g)
        ty = ((torch.arange(M, device=DEV) * 3 + 1) % NTYPE).long()                # differs by row
        cases = []
        for pos in (0, NPOS - 1):
            posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
            cases.append((dict(emb_pos=wpe, emb_type=wte, type_ids=ty, pos=posd), acc + wpe[pos].double()[None, :] + wte[ty].double()))
    else:
        resid = torch.randn(M, N, device=DEV, generator=g)
        kw = dict(resid=resid, act=hip.EPI_TANH if kind == "tanh" else hip.EPI_NONE)
        cases = [(kw, (torch.tanh(acc) if kind == "tanh" else acc) + resid.double())]
    kper = -(-(-(-K // S)) // 64) * 64
    S_eff = -(-K // kper)
    tiles = -(-M // 64) * -(-N // 64)
    bound = 4e-5 * math.sqrt(K) * a.pow(2).mean().sqrt().item() * w.pow(2).mean().sqrt().item()
    for kw, ref in cases:
        ws = torch.full((tiles * S_eff * 4096,), NAN, device=DEV)
        cnt = torch.zeros(tiles * 4, dtype=torch.int32, device=DEV)
        outs = []
        for rep in range(3):
            C = torch.full((M, N), 7.0, device=DEV)
            Cp = _nan_planes(M, N)
            so = torch.full((M, hip.DG_NP, 2), NAN, device=DEV)
            hip.decode_gemm_x3(2, Ap, Wp, M, N, K, C_=C, Cp=Cp, bias=bias, stats_out=so, splits=S, ws=ws, counters=cnt, **kw)
            assert int(cnt.abs().sum()) == 0                      # the counters are zero afterwards
            outs.append((C, Cp, so))
        C, Cp, so = outs[0]
        name = "x3 reduce M=%d K=%d S=%d N=%d %s" % (M, K, S, N, kind)
        err = (C.double() - ref).abs()
        assert (err <= bound + 2.0 ** -22 * ref.abs()).all(), (name, err.max().item(), bound)
        _assert_split(Cp, C, name)
        _stats_check(so, C.double(), N, name)
        npo = N // 32
        for C_, Cp_, so_ in outs[1:]:                                # three repeats are bit-equal
            assert torch.equal(C_, C) and torch.equal(Cp_.t, Cp.t) and torch.equal(so_[:, :npo], so[:, :npo]), name


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("M", [3, 200])
def test_decode_gemm_bf16_embedding_residual(M, S):
    """the bf16 kernel's mode 2 with the GPT-2 input embedding as the residual: A W^T + b + wpe[pos] + wte[type]"""
    K, N, NPOS, NTYPE = 384, 96, 7, 4
    A = rnd(M, K, dtype=BF, seed=M, scale=0.5).to(DEV)
    W = rnd(N, K, dtype=BF, seed=M + 1, scale=0.05).to(DEV)
    bias = rnd(N, seed=M + 2, scale=0.1).to(DEV)
    wpe = rnd(NPOS, N, dtype=BF, seed=M + 3).to(DEV)
    wte = rnd(NTYPE, N, dtype=BF, seed=M + 4).to(DEV)
    ty = ((torch.arange(M, device=DEV) * 3 + 1) % NTYPE).long()
    tiles = -(-M // 64) * -(-N // 64)
    for pos in (0, NPOS - 1):
        posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
        ws = torch.full((tiles * S * 4096,), NAN, device=DEV)
        cnt = torch.zeros(tiles * 4, dtype=torch.int32, device=DEV)
        C = torch.full((M, N), 7.0, device=DEV, dtype=BF)
        so = torch.full((M, hip.DG_NP, 2), NAN, device=DEV)
        hip.decode_gemm(2, A, W, C, M, N, K, bias=bias, stats_out=so, splits=S, ws=ws, counters=cnt, emb_pos=wpe, emb_type=wte,
                        type_ids=ty, pos=posd)
        ref = A.double() @ W.double().t() + bias.double() + wpe[pos].double()[None, :] + wte[ty].double()
        close(C, ref, BF, K, "bf16 embedding residual M=%d S=%d pos=%d" % (M, S, pos))
        assert int(cnt.abs().sum()) == 0
        _stats_check(so, C.double(), N, "bf16 embedding residual")
