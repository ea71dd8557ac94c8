"""Rhyme schemes on the MI355X: the *_rhyme selection entries against the *_tmpl / *_lines entries given the follower's class as a
static end set, the decoders (GreedyDecoder / BeamDecoder with rhyme_scheme=) against the CPU restatements of
tests/test_rhyme_cpu.py, sampling against a host restatement driven by the decoder's own uniforms, composition with prefixes /
bounds / templates / n-gram bans, a whole given leader line, off-means-off, full-size determinism and the text surface.  Every
column of every output row is held to the rule (test_rhyme_cpu.rhyme_violations skips none).

The comparison scheme is tests/test_template_gpu.py's, unchanged: ids equal to the CPU restatement in f32 and bf16x3, the beam
comparison over the length its margins allow with scores to 1e-3, the sampled pick inside its CDF interval to 1e-4 Z."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_lines  # noqa: E402
from mmtg_amd.generate import top_k_top_p_filtering  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case, start_row  # noqa: E402
from test_lines_cpu import CAP, apply_rule, line_rule  # noqa: E402
from test_lines_gpu import device_tables  # noqa: E402
from test_ngram_cpu import banned_ids  # noqa: E402
from test_ngram_gpu import _histories, build, full_size_model  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402
from test_rhyme_cpu import (LENGTH, cpu_rhyme_beam_search, cpu_rhyme_greedy, fixture_rhymes, followers_rhyme, line_end,  # noqa: E402
                            rhyme_ends, rhyme_violations)
from test_template_cpu import content_ids  # noqa: E402

DEV = "cuda"


def device_rhyme(t):
    """check_lines' rhyme tables as the (class_of, lead, distinct) tuple of the hip.decode_*_rhyme bindings."""
    return torch.from_numpy(t.class_of).to(DEV), torch.from_numpy(t.lead).to(DEV), t.distinct


def all_violations(ids, tables, prefixes=None, n=0):
    ids = ids.cpu().tolist()
    out = []
    for b, r in enumerate(ids):
        v = rhyme_violations(r, tables, b, start=len(prefixes[b]) if prefixes else 1, n=n)
        if v:
            out.append((b, v))
    return out


def all_rhyme(ids, tables, row_of=lambda b: b):
    """Every follower of every row whose leader ended on an id with a class rhymes; returns how many there were."""
    count = 0
    for b, r in enumerate(ids.cpu().tolist()):
        pairs = followers_rhyme(r, tables, row_of(b))
        assert all(ok for _, _, ok in pairs), (b, pairs)
        count += len(pairs)
    return count


# ------------------------------------------------------------------ 1. kernels
K1, K2, K3 = frozenset({3, 30, 31, 32}), frozenset({4, 40, 41, 42}), frozenset({5, 50, 51, 52})


def _kernel_case(n, distinct, templates):
    """Eight rows over three lines under "AAA" (rows 0 - 5), "A.A" (row 6) and no scheme (row 7); the histories are random over
    ids 3 .. 5 and PAD, so every leader line ends on a classed id except where the test plants 77 (row 2) or an empty line (row 3)."""
    B, P, V, Vp, Tmax = 8, 5, 160, 168, 64
    g = torch.Generator().manual_seed(700 + n)
    logits = torch.randn(B, Vp, generator=g) * 2
    logits[:, 3:6] += 6.0
    logits[:, 0] += 5.0
    logits[:, 30:53] += 3.0
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24)
    seq0 = _histories(B, P, Tmax, g)
    seq0[2, P + SENT - 2] = 77                                                 # a leader line that ends on an id without a class
    seq0[3, P + 1:P + SENT - 1] = 0                                            # an empty leader line
    seq0[4, P + SENT - 4:P + SENT - 1] = 0                                     # a leader line that ended early: PAD after its last id
    length = Tmax - P - 1                                                      # 58 lyric positions: three lines
    wide = frozenset({3, 4, 5, 30, 40, 50, 60})
    tm = None if not templates else [[(60, None, wide, Ellipsis), (wide, 61, Ellipsis), None], None, [None, (None, wide, Ellipsis), (62, Ellipsis)],
                                     None, None, [(wide,), None, None], None, [(63, Ellipsis)]]
    lens = [[None, (0, 6), (2, 9)], [(0, 12), (0, 3), None], None, [None, (1, 8), None], [None, (0, 5), (0, 4)], [None, (0, 7), (3, 12)],
            [None, None, (0, 6)], [(0, 9)]]
    schemes = ["AAA"] * 6 + ["A.A", None]
    tabs = check_lines(lens, None, B, length, SENT, V, templates=tm, rhyme_scheme=schemes, rhyme_classes=[K1, K2, K3], rhyme_distinct=distinct)
    return B, P, V, Vp, Tmax, length, logits, uni, seq0, tabs, lens, tm


@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("templates", [False, True])
def test_rhyme_entries_equal_the_static_entries_given_the_followers_class_as_an_end_set(n, distinct, templates):
    """At every position each *_rhyme entry writes bit for bit what its *_tmpl (with templates) or *_lines (without: a null table)
    namesake writes on the same logits under tables in which every follower line carries, as a static end set, the set the rule
    finds in the row's history -- the leader's class, with rhyme_distinct minus the group's earlier endings; none where the leader
    gave no class.  Covers sticky-PAD rows, forced columns, held prefix rows, full lines and lines past the scheme."""
    B, P, V, Vp, Tmax, length, logits, uni, seq0, tabs, lens, tm = _kernel_case(n, distinct, templates)
    nb, uni, lg = 4, uni.to(DEV), logits.to(DEV)
    dt, dr = device_tables(tabs), device_rhyme(tabs)
    tmd = None if tabs.tmpl is None else torch.from_numpy(tabs.tmpl).to(DEV)
    kinds = {"follower": 0, "classless": 0, "mask": 0, "removed": 0, "other": 0}
    for pos in (P, P + 8, P + 20, P + 21, P + 22, P + 23, P + 24, P + 26, P + 27, P + 30, P + 33, P + 43, P + 44, P + 45, P + 46,
                P + 48, P + 52, P + 57):
        j = pos + 1 - P
        s0 = seq0.clone()
        s0[5, P + j - 1] = 0                                                   # a sticky-PAD row
        ends = []
        for b in range(B):
            hist = s0[b, P:P + j].tolist()
            row = [tabs.bounds(b, l)[2] for l in range(3)]
            l = j // SENT
            if l < 3 and tabs.leader(b, l) is not None:
                e = rhyme_ends(hist, tabs, b)
                row[l] = e
                if j % SENT not in (0, SENT - 1) and hist[-1] != 0:
                    kinds["follower" if e is not None else "classless"] += 1
                    if e is not None:
                        lo, hi, _ = tabs.bounds(b, l)
                        kinds["mask"] += j % SENT - 1 == hi - 1
                        kinds["removed"] += len(tabs.rhyme_class(line_end(hist, tabs.leader(b, l))) - e)
            else:
                kinds["other"] += 1
            ends.append(row)
        ref = check_lines(lens, ends, B, length, SENT, V, templates=tm)
        assert (ref.lo == tabs.lo).all() and (ref.hi == tabs.hi).all()
        drf = device_tables(ref)
        tmr = None if ref.tmpl is None else torch.from_numpy(ref.tmpl).to(DEV)      # (a class symbol names a row of its own tables' sets)
        s0 = s0.to(DEV)
        for fe in (None, torch.tensor([0, pos + 2, 0, pos + 1, 0, 0, pos + 5, 0], dtype=torch.int32, device=DEV)):
            for kind in ("select", "sample"):
                a, b_ = s0.clone(), s0.clone()
                pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                if kind == "select":
                    if templates:
                        hip.decode_select_tmpl(lg, Vp, V, a, pa[0:1], P, SENT, T, REP, B, drf, tmr, ngram=n, fixed_end=fe, pos_next=pa[1:2])
                    else:
                        hip.decode_select_lines(lg, Vp, V, a, pa[0:1], P, SENT, T, REP, B, drf, ngram=n, fixed_end=fe, pos_next=pa[1:2])
                    hip.decode_select_rhyme(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, B, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe,
                                            pos_next=pb[1:2])
                else:
                    if templates:
                        hip.decode_sample_tmpl(lg, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, drf, tmr, ngram=n, fixed_end=fe,
                                               pos_next=pa[1:2])
                    else:
                        hip.decode_sample_lines(lg, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, drf, ngram=n, fixed_end=fe,
                                                pos_next=pa[1:2])
                    hip.decode_sample_rhyme(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, dr, tmpl=tmd, ngram=n,
                                            fixed_end=fe, pos_next=pb[1:2])
                torch.cuda.synchronize()
                assert int(pb[1]) == pos + 1 == int(pa[1])
                assert torch.equal(a, b_), (pos, kind, fe is None, a[:, pos + 1].tolist(), b_[:, pos + 1].tolist())
            cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
            cvb, cib = cva.clone(), cia.clone()
            pp = torch.tensor([pos], dtype=torch.int32, device=DEV)
            if templates:
                hip.decode_beam_candidates_tmpl(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B, drf, tmr, ngram=n, fixed_end=fe)
            else:
                hip.decode_beam_candidates_lines(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B, drf, ngram=n, fixed_end=fe)
            hip.decode_beam_candidates_rhyme(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cvb, cib, B, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe)
            torch.cuda.synchronize()
            assert torch.equal(cva, cvb) and torch.equal(cia, cib), (pos, fe is None)
    assert min(kinds["follower"], kinds["classless"], kinds["mask"], kinds["other"]) > 0 and (kinds["removed"] > 0) == distinct, kinds


def test_a_scheme_of_dots_through_the_rhyme_entries_is_the_tmpl_entries():
    B, P, V, Vp, Tmax, nb = 8, 5, 160, 168, 64, 4
    g = torch.Generator().manual_seed(23)
    logits = (torch.randn(B, Vp, generator=g) * 2).to(DEV)
    logits[:, 0] += 4.0
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24).to(DEV)
    seq0 = _histories(B, P, Tmax, g).to(DEV)
    E, A = frozenset({4, 5, 40}), frozenset({3, 4, 41})
    args = ([(2, 9), (0, 6)], [None, E], B, 2 * SENT, SENT, V)
    tm = [(A, None, Ellipsis), (None, 60, Ellipsis)]
    base = check_lines(*args, templates=tm)
    for scheme in ("..", "", "AB", [None] * B):
        tabs = check_lines(*args, templates=tm, rhyme_scheme=scheme, rhyme_classes=[K1, K2, K3])
        assert (tabs.lead == -1).all() and (tabs.set_of == base.set_of).all() and (tabs.tmpl == base.tmpl).all()
        dt, db, dr = device_tables(tabs), device_tables(base), device_rhyme(tabs)
        tmd = torch.from_numpy(tabs.tmpl).to(DEV)
        for n in (0, 3):
            for pos in (P, P + 1, P + 7, P + 9, P + 20, P + 21, P + 24, P + 27, P + 30, P + 47):
                a, b_, c_, d_ = (seq0.clone() for _ in range(4))
                pp = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                hip.decode_select_tmpl(logits, Vp, V, a, pp[0:1], P, SENT, T, REP, B, db, tmd, ngram=n, pos_next=pp[1:2])
                hip.decode_select_rhyme(logits, Vp, V, b_, pp[0:1], P, SENT, T, REP, B, dt, dr, tmpl=tmd, ngram=n, pos_next=pp[1:2])
                hip.decode_sample_tmpl(logits, Vp, V, c_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, db, tmd, ngram=n, pos_next=pp[1:2])
                hip.decode_sample_rhyme(logits, Vp, V, d_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, dr, tmpl=tmd, ngram=n,
                                        pos_next=pp[1:2])
                cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
                cvb, cib = cva.clone(), cia.clone()
                hip.decode_beam_candidates_tmpl(logits, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cva, cia, B, db, tmd, ngram=n)
                hip.decode_beam_candidates_rhyme(logits, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cvb, cib, B, dt, dr, tmpl=tmd, ngram=n)
                torch.cuda.synchronize()
                assert torch.equal(a, b_) and torch.equal(c_, d_) and torch.equal(cva, cvb) and torch.equal(cia, cib), (scheme, n, pos)


# ------------------------------------------------------------------ 2. decoders against the CPU restatements
def fixture_args(fx, scheme, distinct):
    classes, bounds = fixture_rhymes(fx)
    kw = dict(line_lengths=bounds, rhyme_scheme=scheme, rhyme_classes=classes, rhyme_distinct=distinct)
    return kw, check_lines(bounds, None, 3, LENGTH, SENT, 160, rhyme_scheme=scheme, rhyme_classes=classes, rhyme_distinct=distinct)


def cut_to(kw, tabs, L):
    """The arguments of a generation of L positions under the rule tabs (made from kw for a longer one) holds for its lines: a leader
    whose followers all lie past L keeps the static end set it has in tabs, given as line_end_ids."""
    nl = (L - 1) // SENT + 1
    scheme = kw["rhyme_scheme"][:nl]
    lone = [l for l, ch in enumerate(scheme) if ch != "." and scheme.count(ch) == 1 and kw["rhyme_scheme"].count(ch) > 1]
    cut = dict(kw, rhyme_scheme="".join("." if l in lone else ch for l, ch in enumerate(scheme)))
    if lone:
        cut["line_end_ids"] = [tabs.bounds(0, l)[2] if l in lone else None for l in range(nl)]
    t = check_lines(cut["line_lengths"], cut.get("line_end_ids"), 3, L, SENT, 160, rhyme_scheme=cut["rhyme_scheme"],
                    rhyme_classes=cut["rhyme_classes"], rhyme_distinct=cut["rhyme_distinct"])
    assert all(t.bounds(b, l) == tabs.bounds(b, l) and t.leader(b, l) == tabs.leader(b, l) for b in range(3) for l in range(nl))
    return cut


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_greedy_under_a_scheme_is_the_cpu_restatement(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    dec = GreedyDecoder(model, 3, max_len=220)
    plain = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP).cpu()
    for scheme, distinct, n in (("AABB", False, 0), ("AABB", True, 3), ("ABAB", False, 3), ("ABAB", True, 0)):
        kw, tabs = fixture_args(fx, scheme, distinct)
        assert len(all_violations(plain, tabs)) == 3                           # the unconstrained run breaks the scheme it then gets
        ids = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, **kw).cpu()
        assert all_violations(ids, tabs, n=n) == [] and all_rhyme(ids, tabs) >= 3
        for row in range(3):
            want, rule = cpu_rhyme_greedy(w, sh, table, start_row(batch, row), LENGTH, tabs, b=row, n=n)
            assert n > 0 or rule.all_banned == 0
            assert ids[row].tolist() == want, (scheme, distinct, n, row)
    assert any("rhyme" in k for k in dec.graphs) and any("distinct" in k for k in dec.graphs)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_four_beams_under_a_scheme_follow_the_cpu_beam_search(mode):
    nb = 4
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    dec = BeamDecoder(model, 3, nb, max_len=LENGTH)
    best = 0
    for scheme, distinct in (("AABB", True), ("ABAB", False)):
        kw, tabs = fixture_args(fx, scheme, distinct)
        lens = []
        for row in range(3):
            _, _, gaps, rule = cpu_rhyme_beam_search(w, sh, table, start_row(batch, row), LENGTH, nb, tabs, b=row)
            assert rule.all_banned == 0
            lens.append(comparable_length(gaps, LENGTH))
        best = max(best, max(lens))
        runs = {}
        for row, L in enumerate(lens):
            if L < 1:
                continue
            if L not in runs:
                runs[L] = [t.cpu() for t in dec.generate(tb, L, temperature=T, repitition_penalty=REP, **cut_to(kw, tabs, L))]
            ids, scores = runs[L]
            cids, cscores, _, rule = cpu_rhyme_beam_search(w, sh, table, start_row(batch, row), L, nb, tabs, b=row)
            assert rule.all_banned == 0
            assert ids[row].tolist() == cids.tolist(), (scheme, row, L)
            np.testing.assert_allclose(scores[row].numpy(), cscores, rtol=0, atol=1e-3)
            for k in range(nb):
                assert rhyme_violations(ids[row, k].tolist(), tabs, row) == []
    assert best >= 40, best


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_one_beam_under_a_scheme_is_greedy_under_the_scheme(mode):
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", mode)
    classes, bounds = fixture_rhymes(fx)
    kw = dict(line_lengths=bounds, rhyme_scheme="AABBAABBAA", rhyme_classes=classes, rhyme_distinct=True)
    tabs = check_lines(bounds, None, 3, 220, SENT, 160, rhyme_scheme="AABBAABBAA", rhyme_classes=classes, rhyme_distinct=True)
    for n in (0, 2):
        args = dict(temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, **kw)
        greedy = GreedyDecoder(model, 3).generate(tb, 220, **args)
        ids, scores = BeamDecoder(model, 3, 1).generate(tb, 220, **args)
        assert torch.equal(ids[:, 0], greedy), n
        assert torch.isfinite(scores).all() and all_violations(greedy, tabs, n=n) == [] and all_rhyme(greedy, tabs) >= 12
    ids, _ = BeamDecoder(model, 3, 4).generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)    # every beam with its own history
    flat = ids.reshape(12, -1)
    assert [r for r in range(12) if rhyme_violations(flat[r].tolist(), tabs, r // 4)] == []
    assert all_rhyme(flat, tabs, row_of=lambda r: r // 4) >= 48


def test_sampling_under_a_scheme_follows_the_host_restatement_with_the_same_uniforms():
    """test_template_gpu's sampling check with the follower's end set taken from the row's own history: the draw is held to the fp32
    rounding of the CDF as there, u Z within 1e-4 Z of the pick's interval."""
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "f32")
    n, top_k, top_p = 3, 10, 0.7
    kw, tabs = fixture_args(fx, "AABB", True)
    dec = GreedyDecoder(model, 3, max_len=LENGTH)
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    steps = []

    def tap(j, with_head, picked, logits):
        if with_head:
            steps.append((j, picked.cpu().tolist(), logits[:, :V].float().cpu().clone(), dec.seq[:, P:P + j].cpu().tolist(),
                          dec.uniforms[P + j - 1].cpu().tolist()))

    ids = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, top_k=top_k, top_p=top_p, no_repeat_ngram_size=n,
                       generator=torch.Generator(device=DEV).manual_seed(11), tap=tap, **kw).cpu()
    assert all_violations(ids, tabs, n=n) == [] and all_rhyme(ids, tabs) >= 4
    checked = followers = 0
    for j, picked, logits, hist, us in steps:
        for b in range(3):
            g = hist[b]
            if g[-1] == 0:
                assert picked[b] == 0
                continue
            lo, hi, e = tabs.bounds(b, j // SENT)
            r = rhyme_ends(g, tabs, b)
            if r is not None:
                e, followers = r, followers + 1
            x = O.process_logits(logits[b], torch.tensor(g), T, REP).clone()
            for v in banned_ids(g, n):
                x[v] = float("-inf")
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
    assert checked > 50 and followers > 10
    again = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, top_k=top_k, top_p=top_p, no_repeat_ngram_size=n,
                         generator=torch.Generator(device=DEV).manual_seed(11), **kw).cpu()
    assert torch.equal(ids, again)


# ------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_schemes_compose_with_a_partial_prefix_bounds_templates_ngram_bans_and_a_whole_given_leader_line(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    cid = content_ids(fx)
    classes, _ = fixture_rhymes(fx)
    A, W = frozenset(cid[0:40:2] + cid[60:64]), frozenset(cid[0:30])           # W meets every rhyme class in seven ids or more
    given = [1, cid[20], cid[21], cid[5]] + [0] * (CAP - 3) + [2]             # a whole leader line of the caller's, ending on cid[5]
    loose = [1, cid[20], cid[60]] + [0] * (CAP - 2) + [2]                     # one ending on an id without a class: line 1 is free
    pre = [given + [1, cid[22]], loose + [1], [1, cid[23]]]                    # + one token of the follower; + none; a partial leader line
    length, n = 4 * SENT, 3
    assert any(cid[5] in k for k in classes) and not any(cid[60] in k for k in classes)
    tm = [[None, (cid[22], None, Ellipsis), (A, Ellipsis), None], None, [(cid[23], A, Ellipsis), None, (None, None, W), (cid[24], Ellipsis)]]
    lens = [[None, (2, 6), (1, 5), (2, 4)], (2, 7), [(3, 8), (2, 9), 3, None]]
    kw = dict(line_lengths=lens, templates=tm, rhyme_scheme=["AABB", "AAB", "ABBA"], rhyme_classes=classes, rhyme_distinct=True,
              no_repeat_ngram_size=n, prefix=pre)
    tabs = check_lines(lens, None, 3, length, SENT, 160, prefix=pre, templates=tm, rhyme_scheme=kw["rhyme_scheme"], rhyme_classes=classes,
                       rhyme_distinct=True)
    ids = GreedyDecoder(model, 3, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, **kw).cpu()
    for b, p in enumerate(pre):
        assert ids[b, :len(p)].tolist() == p
    assert all_violations(ids, tabs, pre, n=n) == []
    rk = next(k for k in classes if cid[5] in k)
    assert line_end(ids[0].tolist(), 1) in rk - {cid[5]}                       # the follower rhymes with the given line, on another id
    assert [l for l, _, _ in followers_rhyme(ids[1].tolist(), tabs, 1)] == []  # a class-less given leader: no rhyme asked of lines 1, 2
    assert all_rhyme(ids, tabs) >= 3
    if mode == "f32":
        for b in range(3):
            want, rule = cpu_rhyme_greedy(w, sh, table, start_row(batch, b), length, tabs, b=b, n=n, prefix=pre[b])
            assert ids[b].tolist() == want, b
    bids, _ = BeamDecoder(model, 3, 4, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, **kw)
    flat = bids.reshape(12, -1).cpu()
    for r in range(12):
        assert flat[r, :len(pre[r // 4])].tolist() == pre[r // 4]
        assert rhyme_violations(flat[r].tolist(), tabs, r // 4, start=len(pre[r // 4]), n=n) == []
    all_rhyme(flat, tabs, row_of=lambda r: r // 4)
    sids = GreedyDecoder(model, 3, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                                                            generator=torch.Generator(device=DEV).manual_seed(2), **kw).cpu()
    assert all_violations(sids, tabs, pre, n=n) == []


# ------------------------------------------------------------------ 4. off means off
def test_rhyme_scheme_none_is_exactly_the_call_without_the_argument(monkeypatch):
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "bf16")
    classes, bounds = fixture_rhymes(fx)
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
    for kw in (dict(), dict(rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False)):
        del names[:]
        dec = GreedyDecoder(model, 3, use_graph=False)
        ids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)
        sids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                            generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        bids, sc = BeamDecoder(model, 3, 4, use_graph=False).generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)
        runs.append((list(names), ids, sids, bids, sc))
        assert dec.rules.rhyme is None and dec.rules.tmpl is None and dec.rules.lines is None
    assert runs[0][0] == runs[1][0] and not any("_rhyme" in x or "_tmpl" in x or "_lines" in x for x in runs[0][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    monkeypatch.undo()
    fresh, dec = GreedyDecoder(model, 3), GreedyDecoder(model, 3)
    a = fresh.generate(tb, 220, temperature=T, repitition_penalty=REP)
    b = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, rhyme_scheme=None)
    assert torch.equal(a, b) and torch.equal(a, runs[0][1]) and set(dec.graphs) == set(fresh.graphs)
    keys = set(dec.graphs)
    c = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, rhyme_scheme="..........", rhyme_classes=classes)   # the *_rhyme entries, nothing asked
    assert torch.equal(a, c) and dec.rules.rhyme is not None
    new = set(dec.graphs) - keys
    assert new and all("rhyme" in k and k[0] for k in new)                     # head steps only; the others replay the graphs they had
    d = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, line_lengths=bounds, rhyme_scheme="AA", rhyme_classes=classes)
    assert not torch.equal(a, d)
    assert torch.equal(dec.generate(tb, 220, temperature=T, repitition_penalty=REP), a) and dec.rules.rhyme is None and dec.rules.lines is None


# ------------------------------------------------------------------ 5. full size
def test_full_size_bf16_under_a_scheme_is_bit_stable_and_rhymes():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    B, Ln, n = 256, 220, 3
    nbt = synth.make_batch(B, mcfg, dcfg, V, seed=13)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    rng = np.random.RandomState(8)
    ids = rng.permutation(np.arange(200, V))[:6000]
    classes = [frozenset(int(v) for v in ids[i::12]) for i in range(12)]       # twelve classes of 500 ids
    schemes = ["AABBAABBAA", "ABABCDCD", "ABCB.ABCB", "AAAAAAAAAA", None, "A.A.A"]
    tabs = check_lines((3, 18), None, B, Ln, SENT, V, rhyme_scheme=[schemes[b % 6] for b in range(B)], rhyme_classes=classes,
                       rhyme_distinct=True)
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
        assert all_rhyme(g1, tabs) > B
        assert int(g1.min()) >= 0 and int(g1.max()) < V
    bd = BeamDecoder(model, 64, 4, max_len=Ln)
    pb = {k: v[:64] for k, v in batch.items()}
    bt = tabs.take(list(range(64)))
    i1, s1 = bd.generate(pb, Ln, temperature=T, repitition_penalty=REP, line_lengths=bt)
    i2, s2 = bd.generate(pb, Ln, temperature=T, repitition_penalty=REP, line_lengths=bt, use_graph=False)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    flat = i1.reshape(256, -1).cpu()
    assert [r for r in range(256) if rhyme_violations(flat[r].tolist(), bt, r // 4)] == []
    assert all_rhyme(flat, bt, row_of=lambda r: r // 4) > 256


# ------------------------------------------------------------------ 6. text surface
def test_generate_samples_and_beams_rhyme_their_lines_under_aabb():
    from mmtg_amd.generate import encode_rhyme_classes, generate_beams, generate_samples
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

        def convert_tokens_to_ids(self, t):
            return ord(t) - 0x4e00 if 0x4e00 <= ord(t) < 0x4e00 + 160 else 100

    tok = Tok()
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    sets, bounds = fixture_rhymes(fx)
    classes = encode_rhyme_classes(tok, ["".join(chr(0x4e00 + v) for v in sorted(k)) for k in sets], vocab_cut=160)
    assert classes == sets
    which = lambda ch: next((i for i, k in enumerate(classes) if ord(ch) - 0x4e00 in k), None)      # noqa: E731
    kw = dict(length=4 * SENT, line_lengths=bounds, rhyme_scheme="AABB", rhyme_classes=classes)
    texts = generate_samples(model, rows, tok, n_samples=4, **kw)                                       # one scheme for all prompts
    assert len(texts) == 3 and all(len(t) == 4 for t in texts)
    for t in texts:
        for s in t:
            parts = s.split("，")
            assert len(parts) == 4 and all(3 <= len(p) <= 8 for p in parts), s
            assert which(parts[0][-1]) is not None and which(parts[0][-1]) == which(parts[1][-1]), s
            assert which(parts[2][-1]) is not None and which(parts[2][-1]) == which(parts[3][-1]), s
    out = generate_beams(model, rows, tok, num_beams=4, return_all=True, rhyme_distinct=True,
                         **dict(kw, rhyme_scheme=["AABB", "ABAB", None]))                               # per prompt
    assert len(out) == 3 and all(len(b) == 4 for b in out)
    for p, (x, y) in ((0, ((0, 1), (2, 3))), (1, ((0, 2), (1, 3)))):
        for text, score in out[p]:
            parts = text.split("，")
            assert len(parts) == 4 and np.isfinite(score)
            for i, k in (x, y):
                assert which(parts[i][-1]) is not None and which(parts[i][-1]) == which(parts[k][-1]) and parts[i][-1] != parts[k][-1], text
