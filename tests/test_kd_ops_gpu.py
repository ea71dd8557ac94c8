"""mmtg_distill_fwd, mmtg_loss_bwd_kd and mmtg_loss_bwd_kd_x3 alone on the GPU against the float64 reference of tests/kd_ref.py
within its derived bounds, on every element.  The host side is in tests/test_kd_cpu.py, the trainer in tests/test_kd_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import kd_ref as R  # noqa: E402
from mmtg_amd import hip  # noqa: E402

DEV = "cuda"
GUARD = 16
SENT = 3.5
F32, BF = torch.float32, torch.bfloat16
# (bf16 rows are 16-byte aligned: the case of odd strides is fp32 on both sides)
CASES = [(g, sbf, tbf) for g in R.geometries() for (sbf, tbf) in ((False, False), (True, True), (False, True), (True, False))
         if g[1] % 8 == 0 or not (sbf or tbf)]


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _within(name, got, ref, allow):
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()) and bool((err <= allow).all()), "%s: %d outside the bound, worst err/allowed %.3g" % (
        name, int((err > allow).sum()), float((err / allow.clamp(min=1e-300)).max()))
    return float((err / allow.clamp(min=1e-300)).max())


class Dev:
    """a case on the device"""

    def __init__(self, geo, sbf, tbf):
        self.V, self.ldl, self.ldt, self.P, self.L = geo
        self.host = R.case(self.V, self.ldl, self.ldt, self.P, self.L, sbf, tbf)
        (self.x, self.lse, self.c, self.u, self.lse_c, self.lse_u, self.tg, self.topic, self.coef) = (t.to(DEV) for t in self.host)
        self.M = R.B * (self.P + self.L)
        self.Vpad = R.padded(self.V)

    def teacher(self, s):
        """(cond, uncond, ldt, lse_c, lse_u, scale) as the bindings take them"""
        return (self.c, None, self.ldt, self.lse_c, None, 1.0) if s is None else (self.c, self.u, self.ldt, self.lse_c, self.lse_u, s)

    def fwd(self, s, teacher=None):
        M = self.M
        outs = [torch.full((n + GUARD,), SENT, device=DEV) for n in (M, M, R.B, 1)]
        c, u, ldt, lc, lu, sc = teacher or self.teacher(s)
        hip.distill_fwd(self.x, self.ldl, c, u, ldt, self.V, self.lse, lc, lu, sc, R.B, self.P, self.L, float(R.B),
                        outs[0][:M], outs[1][:M], outs[2][:R.B], outs[3][:1])
        torch.cuda.synchronize()
        for t, n in zip(outs, (M, M, R.B, 1)):
            assert bool((t[n:] == SENT).all())
        return [t[:n].clone() for t, n in zip(outs, (M, M, R.B, 1))]

    def bwd(self, form, s, kd_lg, w, teacher=None, plain=False, lm_coef=R.LM_COEF):
        """one backward launch in `form` into guarded outputs (eight guard columns behind every row, GUARD words behind the last);
        returns the CPU tensors (out,) or (hi, lo), [M, Vpad].  plain: mmtg_loss_bwd / mmtg_loss_bwd_x3 instead."""
        M, V, Vpad, P, L = self.M, self.V, self.Vpad, self.P, self.L
        c, u, ldt, lc, lu, sc = teacher or self.teacher(s)
        head = (self.x if form != "inplace" else self.x.clone(), self.ldl, V, self.topic, self.tg, self.lse, self.coef, R.GSCALE)
        kdargs = (c, u, ldt, lc, lu, sc, kd_lg, w)
        ldd = Vpad + 8
        if form == "x3":
            flat = torch.full((2 * M * ldd + GUARD,), SENT, device=DEV, dtype=BF)
            planes = hip.Planes(flat, M, Vpad, ld=ldd, plane=M * ldd)
            if plain:
                hip.loss_bwd_x3(*head, R.B, P, L, planes, Vpad, lm_coef=lm_coef)
            else:
                hip.loss_bwd_kd_x3(*head, *kdargs, R.B, P, L, planes, Vpad, lm_coef=lm_coef)
            torch.cuda.synchronize()
            both = flat[:2 * M * ldd].view(2, M, ldd)
            assert bool((flat[2 * M * ldd:] == SENT).all()) and bool((both[:, :, Vpad:] == SENT).all())
            return both[0, :, :Vpad].cpu(), both[1, :, :Vpad].cpu()
        if form == "inplace":
            out = head[0]
            if plain:
                hip.loss_bwd(*head, R.B, P, L, out, self.ldl, Vpad, lm_coef=lm_coef)
            else:
                hip.loss_bwd_kd(*head, *kdargs, R.B, P, L, out, self.ldl, Vpad, lm_coef=lm_coef)
            torch.cuda.synchronize()
            assert torch.equal(_bits(out[:, Vpad:]), _bits(self.x[:, Vpad:]))
            return (out[:, :Vpad].cpu(),)
        flat = torch.full((M * ldd + GUARD,), SENT, device=DEV, dtype=F32 if form == "f32" else BF)
        out = flat[:M * ldd].view(M, ldd)
        if plain:
            hip.loss_bwd(*head, R.B, P, L, out, ldd, Vpad, lm_coef=lm_coef)
        else:
            hip.loss_bwd_kd(*head, *kdargs, R.B, P, L, out, ldd, Vpad, lm_coef=lm_coef)
        torch.cuda.synchronize()
        assert bool((flat[M * ldd:] == SENT).all()) and bool((out[:, Vpad:] == SENT).all())
        return (out[:, :Vpad].cpu(),)

    def forms(self, sbf):
        """the storage forms of d(logits) this student takes: bf16 logits go with bf16 dlogits (also in place); the plane pair reads
        aligned fp32 rows of at least Vpad columns"""
        if sbf:
            return ["bf16", "inplace"]
        return ["f32", "bf16"] + (["x3"] if self.ldl % 4 == 0 and self.ldl >= self.Vpad else [])


@pytest.mark.parametrize("geo,sbf,tbf", CASES, ids=lambda v: "V%d-ldl%d-ldt%d-P%d-L%d" % v if isinstance(v, tuple) else ("bf16" if v else "f32"))
def test_the_entries_against_float64(geo, sbf, tbf):
    d = Dev(geo, sbf, tbf)
    V, P, L, Vpad = d.V, d.P, d.L, d.Vpad
    x, lse, c, u, lse_c, lse_u, tg, topic, coef = d.host
    keep = [t.clone() for t in (d.x, d.c, d.u, d.lse, d.lse_c, d.lse_u, d.tg, d.topic, d.coef)]
    for s in R.SCALES:
        ref = R.forward(x, lse, c, None if s is None else u, lse_c, None if s is None else lse_u, 1.0 if s is None else s, P, L, V, float(R.B))
        row, lg, smp, kd = d.fwd(s)
        worst = [_within(k, got.cpu(), ref[k], ref[a]) for k, a, got in (("kd_row", "allow_row", row), ("kd_lg", "allow_lg", lg),
                                                                        ("kd_sample", "allow_sample", smp))]
        worst.append(_within("kd", kd.cpu()[0], ref["kd"], ref["allow_kd"]))
        rows = ref["rows"]
        assert bool((row.cpu()[~rows] == 0).all()) and bool((lg.cpu()[~rows] == 0).all())
        again = d.fwd(s)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((row, lg, smp, kd), again))          # equal inputs, equal bits
        dref, allow = R.backward(x, lse, ref, topic, tg, coef, R.GSCALE, R.LM_COEF, R.KD_COEF, P, V, Vpad)
        got = {}
        for form in d.forms(sbf):
            out = d.bwd(form, s, lg, R.KD_COEF)
            got[form] = out
            if form == "x3":
                worst.append(_within("d x3", out[0].double() + out[1].double(), dref, R.allow_planes(dref, allow)))
                worst.append(_within("d x3 hi", out[0], dref, R.allow_bf16(dref, allow)))
            elif form == "f32":
                worst.append(_within("d f32", out[0], dref, allow))
            else:
                worst.append(_within("d " + form, out[0], dref, R.allow_bf16(dref, allow)))
            assert all(bool((o[:, V:] == 0).all()) for o in out)                    # pad columns: +0
            out2 = d.bwd(form, s, lg, R.KD_COEF)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, out2)), form
            # kd_coef = 0: the bits of mmtg_loss_bwd / mmtg_loss_bwd_x3
            zero, plain = d.bwd(form, s, lg, 0.0), d.bwd(form, s, lg, 0.0, plain=True)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(zero, plain)), form
        if sbf:
            assert torch.equal(_bits(got["inplace"][0]), _bits(got["bf16"][0]))         # in place or not: the same bits
        print(geo, sbf, tbf, s, "worst err / allowed: " + " ".join("%.3f" % w for w in worst))
    # without the LM rows (lm_coef = 0: rows t < P are zeros) the term is the same on the loss rows
    s = 1.5
    ref = R.forward(x, lse, c, u, lse_c, lse_u, s, P, L, V, float(R.B))
    lg = d.fwd(s)[1]
    dref, allow = R.backward(x, lse, ref, topic, tg, coef, R.GSCALE, 0.0, R.KD_COEF, P, V, Vpad)
    for form in d.forms(sbf):
        out = d.bwd(form, s, lg, R.KD_COEF, lm_coef=0.0)
        val = out[0].double() + out[1].double() if form == "x3" else out[0]
        _within("d %s, lm_coef 0" % form, val, dref, allow if form == "f32" else R.allow_planes(dref, allow) if form == "x3" else R.allow_bf16(dref, allow))
    # cond == uncond bit for bit with equal lse: nothing depends on the scale
    same = [(d.c, d.c.clone(), d.ldt, d.lse_c, d.lse_c.clone(), sc) for sc in (0.0, 7.5)]
    f0, f1 = d.fwd(0.0, same[0]), d.fwd(7.5, same[1])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(f0, f1))
    for form in d.forms(sbf):
        o0, o1 = d.bwd(form, 0.0, f0[1], R.KD_COEF, same[0]), d.bwd(form, 7.5, f1[1], R.KD_COEF, same[1])
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(o0, o1)), form
    for t, k in zip((d.x, d.c, d.u, d.lse, d.lse_c, d.lse_u, d.tg, d.topic, d.coef), keep):
        assert torch.equal(t, k)                                                    # the inputs are unchanged


def test_a_refused_call_writes_nothing():
    geo = (160, 168, 168, 3, 5)
    d = Dev(geo, True, True)
    M, V, P, L, Vpad = d.M, d.V, d.P, d.L, d.Vpad
    outs = [torch.full((n,), SENT, device=DEV) for n in (M, M, R.B, 1)]
    good = dict(logits=d.x, ldl=d.ldl, cond=d.c, uncond=d.u, ldt=d.ldt, V=V, lse=d.lse, lse_c=d.lse_c, lse_u=d.lse_u, scale=2.0, B=R.B, P=P,
                L=L, batch_den=2.0, kd_row=outs[0], kd_lg=outs[1], kd_sample=outs[2], kd=outs[3])
    nan, inf = float("nan"), float("inf")
    keep = [t.clone() for t in (d.c, d.u, d.lse_c)]
    as_rows = lambda t: t.view(-1)[:4 * M].view(torch.float32)[:M] if t.dtype == BF else t.view(-1)[:M]
    for bad in (dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(V=0), dict(ldl=152), dict(ldt=152), dict(ldl=164), dict(B=0),
                dict(P=-1), dict(L=1), dict(batch_den=0.0), dict(batch_den=nan), dict(batch_den=inf), dict(lse=None), dict(kd_lg=None),
                dict(kd_row=as_rows(d.c)), dict(kd_lg=as_rows(d.u)), dict(kd_sample=d.lse_c[:R.B])):
        with pytest.raises(RuntimeError, match="distill_fwd"):
            hip.distill_fwd(**dict(good, **bad))
    with pytest.raises(ValueError):
        hip.distill_fwd(**dict(good, lse_u=None))
    lg = d.fwd(2.0)[1]
    dl = torch.full((M, Vpad), SENT, device=DEV, dtype=BF)
    pl = hip.Planes(torch.full((2, M, Vpad), SENT, device=DEV, dtype=BF), M, Vpad)
    x32 = d.x.float()
    gb = dict(logits=d.x, ldl=d.ldl, V=V, topic_ids=d.topic, targets=d.tg, lse=d.lse, coef=d.coef, gscale=R.GSCALE, cond=d.c, uncond=d.u,
              ldt=d.ldt, lse_c=d.lse_c, lse_u=d.lse_u, scale=2.0, kd_lg=lg, kd_coef=R.KD_COEF, B=R.B, P=P, L=L, dlogits=dl, ldd=Vpad, Vpad=Vpad)
    x3 = dict(gb, logits=x32, planes=pl)
    del x3["dlogits"], x3["ldd"]
    for bad in (dict(scale=-1.0), dict(scale=nan), dict(kd_coef=nan), dict(kd_coef=inf), dict(kd_coef=-0.5), dict(V=0), dict(ldl=152),
                dict(ldt=152), dict(ldt=164), dict(B=0), dict(P=-1), dict(L=1), dict(kd_lg=None), dict(coef=None)):
        with pytest.raises(RuntimeError, match="loss_bwd_kd"):
            hip.loss_bwd_kd(**dict(gb, **bad))
        with pytest.raises(RuntimeError, match="loss_bwd_kd_x3"):
            hip.loss_bwd_kd_x3(**dict(x3, **bad))
    # outputs that touch a teacher input (the lo plane of the second pair would begin inside uncond; it is never dereferenced)
    for bad in (dict(ldl=164), dict(dlogits=d.c.view(-1)[:M * Vpad].view(M, Vpad)), dict(dlogits=d.u.view(-1)[8:8 + M * Vpad].view(M, Vpad))):
        with pytest.raises(RuntimeError, match="loss_bwd_kd"):
            hip.loss_bwd_kd(**dict(gb, **bad))
    for planes in (hip.Planes(d.c, M, Vpad, ld=Vpad, plane=M * Vpad), hip.Planes(pl.t, M, Vpad, ld=Vpad, plane=(d.u.data_ptr() - pl.t.data_ptr()) // 2)):
        if planes.plane % 8 == 0 and planes.plane >= M * Vpad:
            with pytest.raises(RuntimeError, match="loss_bwd_kd_x3"):
                hip.loss_bwd_kd_x3(**dict(x3, planes=planes))
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs) and bool((dl == SENT).all()) and bool((pl.t == SENT).all())
    for t, k in zip((d.c, d.u, d.lse_c), keep):
        assert torch.equal(t, k)
