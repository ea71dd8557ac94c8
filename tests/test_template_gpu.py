"""Line templates on the MI355X: the *_tmpl selection entries against their *_lines namesakes on logits the test has pre-masked,
given columns against the rule whatever the logits, the decoders (GreedyDecoder / BeamDecoder with templates=) against the CPU
restatements of tests/test_template_cpu.py, sampling against a host restatement driven by the decoder's own uniforms, composition
with prefixes / bounds / end sets / n-gram bans, off-means-off, full-size determinism and the text surface.  Every column of every
output row is held to the rule (test_template_cpu.template_violations skips none).

The runs compared with the CPU restatements hold no all-banned column: the restatement counts them (tests/test_template_cpu.py
asserts 0 for these fixtures and templates, and the comparisons here assert it again)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_lines  # noqa: E402
from mmtg_amd.generate import top_k_top_p_filtering  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case, start_row  # noqa: E402
from test_lines_cpu import CAP, apply_rule, line_lengths_of, line_rule  # noqa: E402
from test_lines_gpu import device_tables  # noqa: E402
from test_ngram_cpu import banned_ids  # noqa: E402
from test_ngram_gpu import _histories, build, full_size_model  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402
from test_template_cpu import (content_ids, cpu_template_beam_search, cpu_template_greedy, fixture_templates,  # noqa: E402
                               template_violations)

DEV = "cuda"


def all_violations(ids, tables, prefixes=None, n=0):
    ids = ids.cpu().tolist()
    out = []
    for b, r in enumerate(ids):
        v = template_violations(r, tables, b, start=len(prefixes[b]) if prefixes else 1, n=n)
        if v:
            out.append((b, v))
    return out


def fixture_tables(fx, rows, length):
    kw, A, Bc, ends = fixture_templates(fx)
    return check_lines(kw["line_lengths"][:rows], kw["line_end_ids"][:rows], rows, length, SENT, 160, templates=kw["templates"][:rows]), kw


# ------------------------------------------------------------------ 1. kernels
def _kernel_case(n):
    B, P, V, Vp, Tmax = 8, 5, 160, 168, 64
    g = torch.Generator().manual_seed(500 + n)
    logits = torch.randn(B, Vp, generator=g) * 2
    logits[:, 3:6] += 6.0
    logits[:, 0] += 5.0
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24)
    seq0 = _histories(B, P, Tmax, g)
    A, Bc, E = frozenset({3, 4, 40, 41}), frozenset({4, 5, 50}), frozenset({5, 40})
    tm = [[(A, None, 77, A, Bc, None, None, None, 60, None, A, Ellipsis), (Bc, Bc, Bc, A, 61, Ellipsis)],
          [(None, None, None, Bc, Ellipsis), None],
          [(3, 4, 5, A), (A, 70, None, Bc, A, Bc, None, None, A)],
          None,
          [tuple([A] * 11), (None, None, None, 88, Ellipsis)],
          [(Bc, None, None, A, Ellipsis), (62, Ellipsis)],
          [(A, A, A, A, A, A, A, A, A, A, Bc), tuple([Bc] * 4)],
          [(None,) * 4 + (Ellipsis,), (None, None, None, A, None, None, None, None, Bc)]]
    lens = [[(0, 12), None], None, None, [(0, 3), (5, 20)], None, [(2, 11), None], None, [(0, 11), None]]
    ends = [[None, None], None, [None, E], [E, None], None, [None, E], [E, None], [E, E]]
    tabs = check_lines(lens, ends, B, 2 * SENT, SENT, V, templates=tm)        # two lines: the third is past the tables
    return B, P, V, Vp, Tmax, logits, uni, seq0, tabs


@pytest.mark.parametrize("n", [0, 2, 3])
def test_tmpl_entries_equal_their_lines_namesakes_on_pre_masked_logits_and_write_given_ids(n):
    """On a class column each *_tmpl entry writes bit for bit what its *_lines namesake writes on logits in which the ids outside the
    class were set to -inf beforehand (the penalty, the temperature and the bans keep -inf); on a free column what it writes on the
    logits as they are; on a given column the written id (select, sample) and the offered candidates (the id at 0.0, then id 0 at
    -inf) are the rule's whatever the logits.  Covers sticky-PAD rows, forced columns, held prefix rows, full lines, a class
    meeting an end set, and a line past the tables."""
    B, P, V, Vp, Tmax, logits, uni, seq0, tabs = _kernel_case(n)
    nb, uni = 4, uni.to(DEV)
    dt = device_tables(tabs)
    tm = torch.from_numpy(tabs.tmpl).to(DEV)
    kinds = {"given": 0, "class": 0, "class+set": 0, "free": 0, "full": 0, "ngram": 0}
    for pos in (P, P + 2, P + 3, P + 4, P + 8, P + 10, P + 20, P + 21, P + 22, P + 25, P + 26, P + 30, P + 47):
        j = pos + 1 - P
        s0 = seq0.clone()
        s0[5, P + j - 1] = 0                                                  # a sticky-PAD row
        masked = logits.clone()
        given = {}
        if j % SENT not in (0, SENT - 1):
            for b in range(B):
                hist = s0[b, P:P + j].tolist()
                lo, hi, e = tabs.bounds(b, j // SENT)
                y = tabs.symbol(b, j // SENT, j % SENT - 1)
                if hist[-1] == 0:
                    continue
                r = line_rule(hist, lo, hi, e)
                if r == "pad":
                    kinds["full"] += 1
                    continue
                if isinstance(y, int):
                    given[b] = y
                    kinds["given"] += 1
                elif y is not None:
                    out = [v for v in range(V) if v not in y]
                    masked[b, out] = float("-inf")
                    kinds["class+set" if r[1] is not None else "class"] += 1
                else:
                    kinds["free"] += 1
                kinds["ngram"] += len(banned_ids(hist, n))
        s0, lg, mk = s0.to(DEV), logits.to(DEV), masked.to(DEV)
        for fe in (None, torch.tensor([0, pos + 2, 0, pos + 1, 0, 0, pos + 5, 0], dtype=torch.int32, device=DEV)):
            held = set() if fe is None else {b for b in range(B) if pos + 1 < int(fe[b])}
            for kind in ("select", "sample"):
                a, b_ = s0.clone(), s0.clone()
                pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                if kind == "select":
                    hip.decode_select_lines(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, B, dt, ngram=n, fixed_end=fe, pos_next=pa[1:2])
                    hip.decode_select_tmpl(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, B, dt, tm, ngram=n, fixed_end=fe, pos_next=pb[1:2])
                else:
                    hip.decode_sample_lines(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, ngram=n, fixed_end=fe,
                                            pos_next=pa[1:2])
                    hip.decode_sample_tmpl(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, tm, ngram=n, fixed_end=fe,
                                           pos_next=pb[1:2])
                torch.cuda.synchronize()
                assert int(pb[1]) == pos + 1 == int(pa[1])
                for b in range(B):
                    if b in given and b not in held:
                        assert int(b_[b, pos + 1]) == given[b], (pos, kind, b)
                        a[b, pos + 1] = given[b]
                assert torch.equal(a, b_), (pos, kind, fe is None, a[:, pos + 1].tolist(), b_[:, pos + 1].tolist())
            cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
            cvb, cib = cva.clone(), cia.clone()
            pp = torch.tensor([pos], dtype=torch.int32, device=DEV)
            hip.decode_beam_candidates_lines(mk, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B, dt, ngram=n, fixed_end=fe)
            hip.decode_beam_candidates_tmpl(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cvb, cib, B, dt, tm, ngram=n, fixed_end=fe)
            torch.cuda.synchronize()
            for b in range(B):
                if b in given and b not in held:
                    assert cvb[b].tolist() == [0.0] + [float("-inf")] * (nb - 1) and cib[b].tolist() == [given[b]] + [0] * (nb - 1), (pos, b)
                    cva[b], cia[b] = cvb[b], cib[b]
            assert torch.equal(cva, cvb) and torch.equal(cia, cib), (pos, fe is None)
    assert min(kinds["given"], kinds["class"], kinds["class+set"], kinds["free"], kinds["full"]) > 0 and (n == 0 or kinds["ngram"] > 0), kinds


def test_free_symbols_through_the_tmpl_entries_are_the_lines_entries():
    B, P, V, Vp, Tmax, nb = 8, 5, 160, 168, 64, 4
    g = torch.Generator().manual_seed(19)
    logits = (torch.randn(B, Vp, generator=g) * 2).to(DEV)
    logits[:, 0] += 4.0
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24).to(DEV)
    seq0 = _histories(B, P, Tmax, g).to(DEV)
    E = frozenset({4, 5, 40})
    free = check_lines([(2, 9), (0, 6)], [None, E], B, 2 * SENT, SENT, V, templates=[None, None])
    same = check_lines([(2, 9), (3, 6)], [None, E], B, 2 * SENT, SENT, V, templates=[(None, None, Ellipsis), (None,) * 3 + (Ellipsis,)])
    base = check_lines([(2, 9), (3, 6)], [None, E], B, 2 * SENT, SENT, V)
    assert (free.tmpl == -1).all() and (same.tmpl == -1).all() and (same.lo == base.lo).all()
    for tabs, ref in ((free, check_lines([(2, 9), (0, 6)], [None, E], B, 2 * SENT, SENT, V)), (same, base)):
        dt, dr = device_tables(tabs), device_tables(ref)
        tm = torch.from_numpy(tabs.tmpl).to(DEV)
        for n in (0, 3):
            for pos in (P, P + 1, P + 7, P + 9, P + 20, P + 21, P + 24, P + 27, P + 30, P + 47):
                a, b_, c_, d_ = (seq0.clone() for _ in range(4))
                pp = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                hip.decode_select_lines(logits, Vp, V, a, pp[0:1], P, SENT, T, REP, B, dr, ngram=n, pos_next=pp[1:2])
                hip.decode_select_tmpl(logits, Vp, V, b_, pp[0:1], P, SENT, T, REP, B, dt, tm, ngram=n, pos_next=pp[1:2])
                hip.decode_sample_lines(logits, Vp, V, c_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dr, ngram=n, pos_next=pp[1:2])
                hip.decode_sample_tmpl(logits, Vp, V, d_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, tm, ngram=n, pos_next=pp[1:2])
                cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
                cvb, cib = cva.clone(), cia.clone()
                hip.decode_beam_candidates_lines(logits, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cva, cia, B, dr, ngram=n)
                hip.decode_beam_candidates_tmpl(logits, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cvb, cib, B, dt, tm, ngram=n)
                torch.cuda.synchronize()
                assert torch.equal(a, b_) and torch.equal(c_, d_) and torch.equal(cva, cvb) and torch.equal(cia, cib), (n, pos)


# ------------------------------------------------------------------ 2. decoders against the CPU restatements
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_greedy_under_templates_is_the_cpu_restatement(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    length = 6 * SENT
    tabs, kw = fixture_tables(fx, 3, length)
    dec = GreedyDecoder(model, 3, max_len=220)
    plain = dec.generate(tb, length, temperature=T, repitition_penalty=REP).cpu()
    assert len(all_violations(plain, tabs)) == 3                               # the unconstrained run breaks the templates it then gets
    for n in (0, 3):
        ids = dec.generate(tb, length, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, **kw).cpu()
        assert all_violations(ids, tabs, n=n) == []
        assert [int(ids[0, l * SENT + 1]) for l in range(6)] == [s[0] for s in kw["templates"][0]]
        for row in range(3):
            want, rule = cpu_template_greedy(w, sh, table, start_row(batch, row), length, tabs, b=row, n=n)
            assert rule.all_banned == 0
            assert ids[row].tolist() == want, (n, row)
    assert any("tmpl" in k for k in dec.graphs)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_four_beams_under_templates_follow_the_cpu_beam_search(mode):
    nb, full = 4, 6 * SENT
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    tabs, kw = fixture_tables(fx, 3, full)
    lens = []
    for row in range(3):
        _, _, gaps, rule = cpu_template_beam_search(w, sh, table, start_row(batch, row), full, nb, tabs, b=row)
        assert rule.all_banned == 0
        lens.append(comparable_length(gaps, full))
    assert max(lens) >= 40, lens
    dec = BeamDecoder(model, 3, nb, max_len=full)
    runs = {}
    for row, L in enumerate(lens):
        if L < 1:
            continue
        if L not in runs:
            nl = (L - 1) // SENT + 1
            cut = lambda spec: [None if r is None else r[:nl] for r in spec]          # noqa: E731
            runs[L] = [t.cpu() for t in dec.generate(tb, L, temperature=T, repitition_penalty=REP, line_lengths=cut(kw["line_lengths"]),
                                                     line_end_ids=cut(kw["line_end_ids"]), templates=cut(kw["templates"]))]
        ids, scores = runs[L]
        cids, cscores, _, rule = cpu_template_beam_search(w, sh, table, start_row(batch, row), L, nb, tabs, b=row)
        assert rule.all_banned == 0
        assert ids[row].tolist() == cids.tolist(), (row, L)
        np.testing.assert_allclose(scores[row].numpy(), cscores, rtol=0, atol=1e-3)
        for k in range(nb):
            assert template_violations(ids[row, k].tolist(), tabs, row) == []


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_one_beam_under_templates_is_greedy_under_templates(mode):
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", mode)
    tabs, kw = fixture_tables(fx, 3, 220)
    for n in (0, 2):
        args = dict(temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, **kw)
        greedy = GreedyDecoder(model, 3).generate(tb, 220, **args)
        ids, scores = BeamDecoder(model, 3, 1).generate(tb, 220, **args)
        assert torch.equal(ids[:, 0], greedy), n
        assert torch.isfinite(scores).all() and all_violations(greedy, tabs, n=n) == []
    ids, _ = BeamDecoder(model, 3, 4).generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)    # shared by a prompt's beams
    for b in range(3):
        for k in range(4):
            assert template_violations(ids[b, k].tolist(), tabs, b) == []


def test_sampling_under_templates_follows_the_host_restatement_with_the_same_uniforms():
    """test_lines_gpu's sampling check with the template in the host restatement: a given column's pick is its id; a class column's
    logits lose every id outside the class before the reference's top-k / top-p filter.  The draw is held to the fp32 rounding of
    the CDF as there: u Z within 1e-4 Z of the pick's interval."""
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "f32")
    length, n, top_k, top_p = 6 * SENT, 3, 10, 0.7
    tabs, kw = fixture_tables(fx, 3, length)
    dec = GreedyDecoder(model, 3, max_len=length)
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    steps = []

    def tap(j, with_head, picked, logits):
        if with_head:
            steps.append((j, picked.cpu().tolist(), logits[:, :V].float().cpu().clone(), dec.seq[:, P:P + j].cpu().tolist(),
                          dec.uniforms[P + j - 1].cpu().tolist()))

    ids = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=top_k, top_p=top_p, no_repeat_ngram_size=n,
                       generator=torch.Generator(device=DEV).manual_seed(11), tap=tap, **kw).cpu()
    assert all_violations(ids, tabs, n=n) == []
    checked = given = classes = 0
    for j, picked, logits, hist, us in steps:
        for b in range(3):
            g = hist[b]
            if g[-1] == 0:
                assert picked[b] == 0
                continue
            lo, hi, e = tabs.bounds(b, j // SENT)
            y = tabs.symbol(b, j // SENT, j % SENT - 1)
            x = O.process_logits(logits[b], torch.tensor(g), T, REP).clone()
            for v in banned_ids(g, n):
                x[v] = float("-inf")
            if line_rule(g, lo, hi, e) != "pad":
                if isinstance(y, int):
                    assert picked[b] == y
                    given += 1
                    continue
                if y is not None:
                    x[[v for v in range(1, V) if v not in y]] = float("-inf")
                    classes += 1
            x = apply_rule(x, g, lo, hi, e)
            if x is None or not torch.isfinite(x).any():
                assert picked[b] == 0
                continue
            f = top_k_top_p_filtering(x.clone(), top_k=top_k, top_p=top_p)
            assert torch.isfinite(f[picked[b]]), (j, b, picked[b])
            p = torch.exp(f.double() - f.double().max())
            cdf = torch.cumsum(p, 0)
            Z, target = float(cdf[-1]), us[b] * float(cdf[-1])
            assert float(cdf[picked[b]] - p[picked[b]]) - 1e-4 * Z <= target <= float(cdf[picked[b]]) + 1e-4 * Z, (j, b)
            checked += 1
    assert checked > 100 and given > 5 and classes > 10
    again = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=top_k, top_p=top_p, no_repeat_ngram_size=n,
                         generator=torch.Generator(device=DEV).manual_seed(11), **kw).cpu()
    assert torch.equal(ids, again)


# ------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_templates_compose_with_a_partial_prefix_bounds_an_end_set_and_ngram_bans(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    cid = content_ids(fx)
    A, Bc, ends = frozenset(cid[0:40:2] + cid[60:64]), frozenset(cid[1:41:2] + cid[64:84]), frozenset(cid[1:9])
    line = batch["targets"][0, :SENT].tolist()
    pre = [batch["targets"][0, :SENT + 1].tolist() + [cid[20], cid[0]], [1, cid[21]], [1]]     # a whole line + 2 tokens; 1 token; none
    length, n = 4 * SENT, 3
    tm = [[(77,), (cid[20], A, None, Bc, Ellipsis), (A, Ellipsis), None],
          [(cid[21], None, Bc, Ellipsis), (Bc, A, Bc, A), None, (cid[22], Ellipsis)],
          [(A, Bc, Ellipsis)] * 4]
    lens = [[None, (2, 6), (1, 5), (1, 3)], [(3, 8), None, (2, 4), None], (2, 7)]
    es = [[None, ends, None, ends], [ends], [None, ends]]
    tabs = check_lines(lens, es, 3, length, SENT, 160, prefix=pre, templates=tm)
    with pytest.raises(ValueError, match="its template"):
        GreedyDecoder(model, 3, max_len=length).begin(tb, length, prefix=pre, templates=[[None, (cid[23],)], None, None])
    ids = GreedyDecoder(model, 3, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, prefix=pre, line_lengths=lens,
                                                           line_end_ids=es, templates=tm, no_repeat_ngram_size=n).cpu()
    for b, p in enumerate(pre):
        assert ids[b, :len(p)].tolist() == p
    assert all_violations(ids, tabs, pre, n=n) == []
    got = [line_lengths_of(r) for r in ids.tolist()]
    assert 4 <= got[0][1] <= 6 and got[1][1] == 4 and int(ids[1, 3 * SENT + 1]) == cid[22] and got[0][0] == sum(1 for v in line[1:-1] if v != 0)
    if mode == "f32":
        for b in range(3):
            want, rule = cpu_template_greedy(w, sh, table, start_row(batch, b), length, tabs, b=b, n=n, prefix=pre[b])
            assert rule.all_banned == 0 and ids[b].tolist() == want, b
    bids, _ = BeamDecoder(model, 3, 4, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, prefix=pre, line_lengths=lens,
                                                                line_end_ids=es, templates=tm, no_repeat_ngram_size=n)
    flat = bids.reshape(12, -1).cpu()
    for r in range(12):
        assert flat[r, :len(pre[r // 4])].tolist() == pre[r // 4]
        assert template_violations(flat[r].tolist(), tabs, r // 4, start=len(pre[r // 4]), n=n) == []
    kw = dict(temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, prefix=pre, line_lengths=lens, line_end_ids=es, templates=tm,
              no_repeat_ngram_size=n)
    sids = GreedyDecoder(model, 3, max_len=length).generate(tb, length, generator=torch.Generator(device=DEV).manual_seed(2), **kw).cpu()
    assert all_violations(sids, tabs, pre, n=n) == []


# ------------------------------------------------------------------ 4. off means off
def test_templates_none_is_exactly_the_call_without_the_argument(monkeypatch):
    model, tb = build("tiny_s5", "bf16")
    names = []
    real = hip.lib()

    class Lib:
        def __getattr__(self, name):
            f = getattr(real, name)
            if name.startswith("mmtg_decode_select") or name.startswith("mmtg_decode_sample") or name.startswith("mmtg_decode_beam"):
                def entry(*a):
                    names.append(name)
                    return f(*a)
                return entry
            return f
    rec = Lib()
    monkeypatch.setattr(hip, "lib", lambda: rec)
    runs = []
    for kw in (dict(), dict(templates=None)):
        del names[:]
        dec = GreedyDecoder(model, 3, use_graph=False)
        ids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)
        sids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                            generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        bids, sc = BeamDecoder(model, 3, 4, use_graph=False).generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)
        runs.append((list(names), ids, sids, bids, sc))
        assert dec.rules.tmpl is None and dec.rules.lines is None
    assert runs[0][0] == runs[1][0] and not any("_tmpl" in x or "_lines" in x for x in runs[0][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    monkeypatch.undo()
    fresh, dec = GreedyDecoder(model, 3), GreedyDecoder(model, 3)
    a = fresh.generate(tb, 220, temperature=T, repitition_penalty=REP)
    b = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, templates=None)
    assert torch.equal(a, b) and torch.equal(a, runs[0][1]) and set(dec.graphs) == set(fresh.graphs)
    c = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, templates=[None])           # the *_tmpl entries, nothing asked
    assert torch.equal(a, c) and any("tmpl" in k for k in dec.graphs) and dec.rules.tmpl is not None
    d = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, templates=[(50, Ellipsis)])
    assert int(d[0, 1]) == 50 and not torch.equal(a, d)
    assert torch.equal(dec.generate(tb, 220, temperature=T, repitition_penalty=REP), a) and dec.rules.tmpl is None and dec.rules.lines is None


# ------------------------------------------------------------------ 5. full size
def test_full_size_bf16_under_templates_is_bit_stable():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    B, Ln, n = 256, 220, 3
    nbt = synth.make_batch(B, mcfg, dcfg, V, seed=13)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    rng = np.random.RandomState(6)
    sets = [frozenset(int(v) for v in rng.choice(np.arange(200, V), size=k, replace=False)) for k in (20, 40, 700, 3000)]
    tm, lens, ends = [], [], []
    for b in range(B):
        row, ll, ee = [], [], []
        for l in range(10):
            k = int(rng.randint(1, 9))
            syms = tuple([int(rng.randint(200, V)), None, sets[rng.randint(4)]][rng.randint(3)] for _ in range(k))
            kind = rng.randint(3)                                              # none / closed / open
            row.append(None if kind == 0 else syms if kind == 1 else syms + (Ellipsis,))
            ll.append(None if kind == 1 else (int(rng.randint(0, 4)), int(rng.randint(9, CAP + 1))))
            ee.append(sets[3] if (kind != 1 and l % 2) else None)
        tm.append(row)
        lens.append(ll)
        ends.append(ee)
    tm[5], lens[5], ends[5] = None, None, None                                 # an unconstrained row among them
    tabs = check_lines(lens, ends, B, Ln, SENT, V, templates=tm)
    dec = GreedyDecoder(model, B, max_len=Ln, lanes=1)
    assert dec.fused and dec.use_graph
    two = GreedyDecoder(model, B, max_len=Ln, lanes=2)
    plain = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP)
    assert len(all_violations(plain, tabs)) > B // 2
    for kw in (dict(), dict(top_k=10, top_p=0.7)):
        gen = lambda: torch.Generator(device=DEV).manual_seed(21) if kw else None     # noqa: E731
        args = dict(temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, line_lengths=tabs, **kw)
        g1 = dec.generate(batch, Ln, generator=gen(), **args)
        assert torch.equal(dec.generate(batch, Ln, generator=gen(), **args), g1), kw
        assert torch.equal(dec.generate(batch, Ln, generator=gen(), use_graph=False, **args), g1), kw
        assert torch.equal(two.generate(batch, Ln, generator=gen(), **args), g1), kw
        assert all_violations(g1, tabs, n=n) == [], kw
        assert int(g1.min()) >= 0 and int(g1.max()) < V
        if not kw:
            assert torch.equal(g1[5], dec.generate(batch, Ln, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n)[5])
    bd = BeamDecoder(model, 64, 4, max_len=Ln)
    pb = {k: v[:64] for k, v in batch.items()}
    bt = tabs.take(list(range(64)))
    i1, s1 = bd.generate(pb, Ln, temperature=T, repitition_penalty=REP, line_lengths=bt)
    i2, s2 = bd.generate(pb, Ln, temperature=T, repitition_penalty=REP, line_lengths=bt, use_graph=False)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    flat = i1.reshape(256, -1).cpu().tolist()
    assert [r for r in range(256) if template_violations(flat[r], bt, r // 4)] == []


# ------------------------------------------------------------------ 6. text surface
def test_generate_samples_and_beams_open_their_lines_with_the_acrostic_characters():
    from mmtg_amd.generate import encode_line_end, encode_template, generate_beams, generate_samples
    model, tb = build("tiny_s5", "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

        def convert_tokens_to_ids(self, t):
            return ord(t) - 0x4e00 if 0x4e00 <= ord(t) < 0x4e00 + 160 else 100

    tok = Tok()
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    heads = "".join(chr(0x4e00 + v) for v in (50, 61, 72, 83))
    acro = [encode_template(tok, c + "…", vocab_cut=160) for c in heads]
    assert acro[0] == (50, Ellipsis)
    texts = generate_samples(model, rows, tok, n_samples=4, length=4 * SENT, templates=acro)          # one for all prompts
    assert len(texts) == 3 and all(len(t) == 4 for t in texts)
    for t in texts:
        for s in t:
            parts = s.split("，")
            assert len(parts) == 4 and [p[0] for p in parts] == list(heads), s
    level = encode_line_end(tok, "".join(chr(0x4e00 + v) for v in range(30, 60)), vocab_cut=160)
    fill = encode_template(tok, heads[1] + "??L" + heads[2], classes={"L": level}, vocab_cut=160)
    per = [acro, [fill] * 4, None]                                                                      # per prompt
    out = generate_beams(model, rows, tok, num_beams=4, length=4 * SENT, templates=per, return_all=True)
    assert len(out) == 3 and all(len(b) == 4 for b in out)
    for text, score in out[0]:
        assert [p[0] for p in text.split("，")] == list(heads) and np.isfinite(score)
    for text, _ in out[1]:
        parts = text.split("，")
        assert len(parts) == 4
        for p in parts:
            assert len(p) == 5 and p[0] == heads[1] and p[4] == heads[2] and 30 <= ord(p[3]) - 0x4e00 < 60, p
