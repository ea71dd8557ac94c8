"""mmtg_experience_drop and mmtg_guided_loss alone on the GPU: the codes against the numpy restatement and the rows against
hip.cast_f32_to, and the guided cross-entropy against the float64 reference of tests/cfg_ref.py within its derived bounds, on every
element.  The host side is in tests/test_cfg_cpu.py, the trainer in tests/test_cfg_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_ref as R  # noqa: E402
from mmtg_amd import hip  # noqa: E402

DEV = "cuda"
T32 = 1 << 32
GUARD = 16


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _drop(img, txt, B, n, dtype, seed, thr, off=0):
    """one call into guarded outputs; `off` shifts every base by that many elements (misaligned rows).  Returns the outputs, the
    codes and the guards."""
    sent = 3.5
    bufs = [torch.full((off + B * n + GUARD,), sent, device=DEV, dtype=dtype) for _ in range(2)]
    code = torch.full((B + GUARD,), -7, device=DEV, dtype=torch.int32)
    oi, ot = (b[off:off + B * n] for b in bufs)
    hip.experience_drop(img, txt, oi, ot, code[:B], B, n, seed, thr)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[off + B * n:] == sent).all()) and bool((b[:off] == sent).all())
    assert bool((code[B:] == -7).all())
    return oi.view(B, n), ot.view(B, n), code[:B].cpu().numpy()


def _check_drop(B, n, dtype, seed, thr, off=0):
    gen = torch.Generator().manual_seed(B * 100003 + n)
    src = [(torch.randn(off + B * n, generator=gen) * 3.0).to(DEV) for _ in range(2)]
    img, txt = (s[off:] for s in src)
    keep = [s.clone() for s in src]
    oi, ot, code = _drop(img, txt, B, n, dtype, seed, thr, off)
    want = R.codes(seed, B, thr)
    assert np.array_equal(code, want), (B, n, seed, thr)
    for ch, (s, o) in enumerate(((img, oi), (txt, ot))):
        cast = torch.empty(B * n, device=DEV, dtype=dtype)
        hip.cast_f32_to(s.contiguous(), cast, B * n)
        dropped = torch.from_numpy(((want >> ch) & 1).astype(bool))
        ob, cb = _bits(o).view(B, n), _bits(cast).view(B, n)
        assert torch.equal(ob[~dropped], cb[~dropped]), (B, n, ch)
        assert bool((ob[dropped] == 0).all()), (B, n, ch)                 # +0.0 bits, not -0.0
    for s, k in zip(src, keep):
        assert torch.equal(_bits(s), _bits(k))                            # the sources are unchanged
    oi2, ot2, code2 = _drop(img, txt, B, n, dtype, seed, thr, off)
    assert torch.equal(_bits(oi), _bits(oi2)) and torch.equal(_bits(ot), _bits(ot2)) and np.array_equal(code, code2)
    return want


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_experience_drop(dtype, B):
    mixed = R.thresholds(R.MIXED)
    for i, n in enumerate((1, 7, 8, 9, 255, 256, 257, 10240)):
        seed = R.KERNEL_SEEDS[i % 3]
        assert not _check_drop(B, n, dtype, seed, (0, 0, 0)).any()
        assert bool((_check_drop(B, n, dtype, seed, (T32, T32, T32)) == 3).all())
        got = _check_drop(B, n, dtype, seed, mixed)
        if B >= 63:
            assert set(np.unique(got)) == {0, 1, 2, 3}
    # single-channel events and bases that are not 16-byte aligned (the one-element path on a row length the vector path would take)
    assert bool((_check_drop(B, 8, dtype, 1, (0, T32, T32)) == 1).all()) and bool((_check_drop(B, 8, dtype, 1, (0, 0, T32)) == 2).all())
    _check_drop(B, 256, dtype, 0xDEADBEEF, mixed, off=1)


@pytest.mark.parametrize("seed", R.KERNEL_SEEDS)
def test_experience_drop_counts_on_65536_rows(seed):
    B, n = 65536, 8
    thr = R.thresholds(R.MIXED)
    img = torch.randn(B * n, device=DEV)
    oi, ot, code = _drop(img, img.clone(), B, n, torch.bfloat16, seed, thr)
    want = R.codes(seed, B, thr)
    assert np.array_equal(code, want)
    for c, p in ((3, 0.25), (1, 0.10), (2, 0.15)):
        cnt = int((code == c).sum())
        assert cnt == int((want == c).sum()) and abs(cnt - B * p) <= 5.0 * np.sqrt(B * p * (1 - p))
    zi = (oi.float().abs().sum(1) == 0).cpu().numpy()
    zt = (ot.float().abs().sum(1) == 0).cpu().numpy()
    assert np.array_equal(zi, (want & 1) == 1) and np.array_equal(zt, (want & 2) == 2)


# ---------------------------------------------------------------- mmtg_guided_loss
def _guided(c, u, lse_c, lse_u, tg, ldl, V, P, L, scales, topic=True):
    K, M = len(scales), R.B * (P + L)
    nll = torch.full((K * M + GUARD,), 9.5, device=DEV)
    smp = torch.full((K * R.B + GUARD,), 9.5, device=DEV)
    ce = torch.full((K + GUARD,), 9.5, device=DEV)
    tp = torch.zeros(R.B, max(P, 1), dtype=torch.long, device=DEV) if topic else None
    hip.guided_loss(c, u, ldl, V, lse_c, lse_u, tp, tg, scales, R.B, P, L, float(R.B), nll, smp, ce)
    torch.cuda.synchronize()
    for t, n in ((nll, K * M), (smp, K * R.B), (ce, K)):
        assert bool((t[n:] == 9.5).all())
    return nll[:K * M].view(K, M).cpu(), smp[:K * R.B].view(K, R.B).cpu(), ce[:K].cpu()


def _within(name, got, ref, allow):
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()) and bool((err <= allow).all()), "%s: %d outside the bound, worst err/allowed %.3g" % (
        name, int((err > allow).sum()), float((err / allow.clamp(min=1e-300)).max()))
    return float((err / allow.clamp(min=1e-300)).max())


@pytest.mark.parametrize("geo", R.geometries(), ids=lambda g: "V%d-ld%d-P%d-L%d-%s" % (g[:4] + ("bf16" if g[4] else "f32",)))
def test_guided_loss(geo):
    V, ldl, P, L, bf = geo
    c, u, lse_c, lse_u, tg = R.case(*geo)
    dc, du, dlc, dlu, dtg = (t.to(DEV) for t in (c, u, lse_c, lse_u, tg))
    keep = [t.clone() for t in (dc, du)]
    rows = R.loss_rows(R.B, P, L)
    for scales in R.KSETS:
        ref = R.reference(c, u, lse_c, lse_u, tg, P, V, scales, float(R.B))
        nll, smp, ce = _guided(dc, du, dlc, dlu, dtg, ldl, V, P, L, scales)
        worst = [_within("nll", nll, ref["nll"], ref["allow_nll"]), _within("sample_ce", smp, ref["sample_ce"], ref["allow_sample"]),
                 _within("ce", ce, ref["ce"], ref["allow_ce"])]
        print(geo, len(scales), "worst err / allowed: nll %.3f sample_ce %.3f ce %.3f" % tuple(worst))
        assert bool((nll[:, ~rows] == 0).all())
        n2, s2, c2 = _guided(dc, du, dlc, dlu, dtg, ldl, V, P, L, scales, topic=False)        # again, without topic_ids: equal bits
        assert torch.equal(_bits(nll), _bits(n2)) and torch.equal(_bits(smp), _bits(s2)) and torch.equal(_bits(ce), _bits(c2))
        # equal scales give equal bits (slots 1 and 5, 0 and 6, 2 ... of the eight)
        for i in range(len(scales)):
            for j in range(i):
                if scales[i] == scales[j]:
                    assert torch.equal(_bits(nll[i]), _bits(nll[j])) and torch.equal(_bits(ce[i]), _bits(ce[j]))
        # uncond == cond: g_k = lu at every scale, all K results are the same bits, and they are the plain cross-entropy
        ne, se, cee = _guided(dc, dc.clone(), dlc, dlc.clone(), dtg, ldl, V, P, L, scales)
        for k in range(1, len(scales)):
            assert torch.equal(_bits(ne[k]), _bits(ne[0])) and torch.equal(_bits(se[k]), _bits(se[0])) and torch.equal(_bits(cee[k]), _bits(cee[0]))
        same = R.reference(c, c, lse_c, lse_c, tg, P, V, [1.0], float(R.B))
        _within("nll at uncond == cond", ne[:1], same["nll"], same["allow_nll"])
    for t, k in zip((dc, du), keep):
        assert torch.equal(_bits(t), _bits(k))


def test_training_and_decoding_mean_the_same_distribution():
    """L(out) - out[label] with out from hip.decode_guidance on the same two rows and scale, against nll from mmtg_guided_loss,
    within the two bounds (cfg_ref.decode_allow for the decode entry, which computes the rows' log-sum-exps itself)"""
    V, P, L = 13317, 3, 5
    ldl = R.padded(V)
    c, u, lse_c, lse_u, tg = R.case(V, ldl, P, L, False)
    dc, du = c.to(DEV), u.to(DEV)
    M = R.B * (P + L)
    rows = R.loss_rows(R.B, P, L)
    lab = R.row_labels(tg, P, V)
    for s in (0.0, 1.0, 1.5, 7.5):
        ref = R.reference(c, u, lse_c, lse_u, tg, P, V, [s], float(R.B))
        nll, _, _ = _guided(dc, du, lse_c.to(DEV), lse_u.to(DEV), tg.to(DEV), ldl, V, P, L, [s])
        out = torch.zeros(M, ldl, device=DEV)
        hip.decode_guidance(dc, du, ldl, V, s, out, M)
        o = out[:, :V].cpu().double()
        dec = torch.logsumexp(o, 1) - o.gather(1, lab[:, None])[:, 0]
        allow = ref["allow_nll"][0] + 2.0 * (ref["dg_max"][0] + R.decode_allow(c, u, V, s))
        err = (nll[0].double() - dec).abs()[rows]
        print("scale %.1f: worst |nll - decode| %.3e, allowed %.3e" % (s, float(err.max()), float(allow[rows].min())))
        assert bool((err <= allow[rows]).all())
