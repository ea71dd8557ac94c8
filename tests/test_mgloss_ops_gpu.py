"""mmtg_guided_loss_multi alone on the GPU: the per-modality guided cross-entropy against the float64 reference of tests/mgl_ref.py
within its derived bounds, on every row of every case, and the bit-level properties include/mmtg_hip.h states.  The host side is in
tests/test_mgloss_cpu.py, the trainer in tests/test_mgloss_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_ref  # noqa: E402
import mg_ref  # noqa: E402
import mgl_ref as R  # noqa: E402
from mmtg_amd import hip  # noqa: E402

DEV = "cuda"
GUARD = 16


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _device(x, off=0):
    """x on the device, its base `off` bytes behind a 16-byte boundary (fp32 only), beside the whole allocation"""
    if not off:
        return x.to(DEV).contiguous(), None
    assert x.dtype == torch.float32 and off % 4 == 0
    whole = torch.full((x.numel() + 8,), 7e3, device=DEV)
    view = whole[off // 4:off // 4 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == off
    return view, whole


def _multi(mats, lses, tg, ldl, V, P, L, tuples):
    G, M = len(tuples), R.B * (P + L)
    nll = torch.full((G * M + GUARD,), 9.5, device=DEV)
    smp = torch.full((G * R.B + GUARD,), 9.5, device=DEV)
    ce = torch.full((G + GUARD,), 9.5, device=DEV)
    hip.guided_loss_multi(list(mats), list(lses), ldl, V, tg, tuples, R.B, P, L, float(R.B), nll, smp, ce)
    torch.cuda.synchronize()
    for t, n in ((nll, G * M), (smp, G * R.B), (ce, G)):
        assert bool((t[n:] == 9.5).all())                           # the guard words behind each output
    return nll[:G * M].view(G, M).cpu(), smp[:G * R.B].view(G, R.B).cpu(), ce[:G].cpu()


def _within(name, got, ref, allow):
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()) and bool((err <= allow).all()), "%s: %d outside the bound, worst err/allowed %.3g" % (
        name, int((err > allow).sum()), float((err / allow.clamp(min=1e-300)).max()))
    return float((err / allow.clamp(min=1e-300)).max())


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("geo", R.geometries(), ids=R.geo_id)
def test_guided_loss_multi(geo, K):
    V, ldl, P, L, bf, off = geo
    mats, lses, tg = R.case(V, ldl, P, L, bf, K)
    offs = R.offsets(K, off)
    placed = [_device(x, o) for x, o in zip(mats, offs)]
    dm, dl, dtg = [p[0] for p in placed], [l.to(DEV) for l in lses], tg.to(DEV)
    keep = [(p[1] if p[1] is not None else p[0]).clone() for p in placed]
    rows = cfg_ref.loss_rows(R.B, P, L)
    ones = (1.0,) * (K - 1)
    ones_bits = None
    for tuples in R.tuple_sets(K):
        ref = R.reference(mats, lses, tg, P, V, tuples, float(R.B), offs)
        got = _multi(dm, dl, dtg, ldl, V, P, L, tuples)
        nll, smp, ce = got
        worst = [_within("nll", nll, ref["nll"], ref["allow_nll"]), _within("sample_ce", smp, ref["sample_ce"], ref["allow_sample"]),
                 _within("ce", ce, ref["ce"], ref["allow_ce"])]
        print(R.geo_id(geo), "K", K, "G", len(tuples), "worst err / allowed: nll %.3f sample_ce %.3f ce %.3f" % tuple(worst))
        assert bool((nll[:, ~rows] == 0).all())
        assert _same(got, _multi(dm, dl, dtg, ldl, V, P, L, tuples))                    # a second identical call: equal bits
        for i in range(len(tuples)):                                                    # equal tuples give equal bits
            for j in range(i):
                if tuples[i] == tuples[j]:
                    assert _same([nll[i], smp[i], ce[i]], [nll[j], smp[j], ce[j]])
            if tuples[i] == ones:                                                       # every all-ones tuple, of every set, gives one result
                if ones_bits is None:
                    ones_bits = [nll[i], smp[i], ce[i]]
                    plain = cfg_ref.reference(mats[0], mats[0], lses[0], lses[0], tg, P, V, [1.0], float(R.B))
                    _within("nll at all ones against the plain cross-entropy", nll[i:i + 1], plain["nll"], plain["allow_nll"])
                assert _same([nll[i], smp[i], ce[i]], ones_bits)
        # a negative equal to matrix 0, with equal lse, vanishes at any scale: the bits of the launch without it, at K - 1
        # (every position of the K - 1 negatives in turn; at K = 2 nothing is left to launch, so all G results are the all-ones bits)
        for k in range(1, K):
            if off is not None and k == K - 1:
                continue                # (the misaligned matrix is what would be replaced: the launch without it takes the other path)
            m2, l2 = list(dm), list(dl)
            m2[k], l2[k] = dm[0], dl[0]
            eq = _multi(m2, l2, dtg, ldl, V, P, L, tuples)
            if K > 2:
                less = _multi(m2[:k] + m2[k + 1:], l2[:k] + l2[k + 1:], dtg, ldl, V, P, L, [t[:k - 1] + t[k:] for t in tuples])
                assert _same(eq, less), ("branch %d equal to matrix 0" % k)
            else:
                assert all(_same([eq[0][g]], [eq[0][0]]) for g in range(len(tuples)))
        # scale 1 on one branch: the nll bits of the launch without that branch
        if K > 2:
            for k in range(1, K):
                if off is not None and k == K - 1:
                    continue
                t1 = [t[:k - 1] + (1.0,) + t[k:] for t in tuples]
                full = _multi(dm, dl, dtg, ldl, V, P, L, t1)
                less = _multi(dm[:k] + dm[k + 1:], dl[:k] + dl[k + 1:], dtg, ldl, V, P, L, [t[:k - 1] + t[k:] for t in tuples])
                assert _same(full, less), ("scale 1 on branch %d" % k)
        # K = 2 is mmtg_guided_loss's rule up to rounding: within the sum of both allowances
        if K == 2 and off is None:
            scales = [t[0] for t in tuples]
            old = cfg_ref.reference(mats[0], mats[1], lses[0], lses[1], tg, P, V, scales, float(R.B))
            G, M = len(scales), R.B * (P + L)
            o_nll, o_smp, o_ce = (torch.empty(n, device=DEV) for n in (G * M, G * R.B, G))
            hip.guided_loss(dm[0], dm[1], ldl, V, dl[0], dl[1], None, dtg, scales, R.B, P, L, float(R.B), o_nll, o_smp, o_ce)
            for name, a, b, key, allow in (("nll", nll, o_nll.view(G, M), "nll", "allow_nll"), ("ce", ce, o_ce, "ce", "allow_ce")):
                err = (a.double() - b.cpu().double()).abs()
                assert bool((err <= ref[allow] + old[allow]).all()), name
    assert ones_bits is not None
    for p, k in zip(placed, keep):
        assert torch.equal(_bits(p[1] if p[1] is not None else p[0]), _bits(k))         # the inputs (and what lies around them) unchanged


def test_training_and_decoding_mean_the_same_distribution():
    """L(out) - out[label] with out from hip.decode_guidance_multi on the same K rows and scales, against nll from
    mmtg_guided_loss_multi, within the two bounds (mg_ref.multi_allow for the decode entry, which computes the rows' log-sum-exps
    itself; a common shift of a row's scores leaves L(g) - g[label] unchanged, so the lse the training side is given costs nothing)"""
    V, P, L, K = 13317, 3, 5, 4
    ldl = R.padded(V)
    mats, lses, tg = R.case(V, ldl, P, L, False, K)
    M = R.B * (P + L)
    rows = cfg_ref.loss_rows(R.B, P, L)
    lab = cfg_ref.row_labels(tg, P, V)
    dm, dl = [x.to(DEV) for x in mats], [l.to(DEV) for l in lses]
    stacked = torch.cat(dm, 0).contiguous()                         # branch k of row m in row k M + m
    x = np.stack([m_[:, :V].numpy() for m_ in mats])                # float32 [K, M, V]
    for t in [(1.5, 3.0, 0.5), (0.0, 0.0, 0.0), (7.5, 1.0, 3.0), (1.0, 1.0, 1.0)]:
        ref = R.reference(mats, lses, tg, P, V, [t], float(R.B))
        nll, _, _ = _multi(dm, dl, tg.to(DEV), ldl, V, P, L, [t])
        out = torch.zeros(M, ldl, device=DEV)
        hip.decode_guidance_multi(stacked, ldl, V, t, out, M)
        o = out[:, :V].cpu().double()
        dec = torch.logsumexp(o, 1) - o.gather(1, lab[:, None])[:, 0]
        allow = ref["allow_nll"][0] + 2.0 * torch.from_numpy(mg_ref.multi_allow(x, t))
        err = (nll[0].double() - dec).abs()[rows]
        print("scales %r: worst |nll - decode| %.3e, allowed %.3e" % (t, float(err.max()), float(allow[rows].min())))
        assert bool((err <= allow[rows]).all())
