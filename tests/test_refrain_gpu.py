"""Refrain schemes on the MI355X: the *_refrain selection entries against the *_rhyme entries (the source's id on copy columns, the
rhyme entries' output bit for bit everywhere else, with and without logits), the decoders (GreedyDecoder / BeamDecoder with
refrain_scheme=) on their own output and against the CPU restatement of tests/test_refrain_cpu.py, head skipping against the run
that keeps the head, composition with a prefix / bounds / a template / a rhyme scheme / token log-probabilities, off-means-off and
full-size determinism.  Every comparison is on integer ids (candidate values as raw bits), so no tolerance is involved -- except the
log-probabilities of the composition test, held to tests/test_logprob_gpu.py's bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import _check_constraints  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_lines  # noqa: E402
from mmtg_amd.generate import score_sequences  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case, start_row  # noqa: E402
from test_lines_cpu import CAP  # noqa: E402
from test_lines_gpu import device_tables  # noqa: E402
from test_logprob_gpu import PARITY  # noqa: E402
from test_ngram_gpu import _histories, build, full_size_model  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402
from test_refrain_cpu import copies_hold, cpu_refrain_greedy, lines_of, ngram_violations  # noqa: E402
from test_rhyme_cpu import LENGTH, fixture_rhymes, followers_rhyme, rhyme_violations  # noqa: E402
from test_rhyme_gpu import _kernel_case, device_rhyme  # noqa: E402
from test_template_cpu import content_ids  # noqa: E402

DEV = "cuda"
NEG = float("-inf")


def refrain_tables(sh, rows, length, scheme, n=0, **kw):
    """The checked tables of a generation of `rows` rows under refrain_scheme=scheme (and kw: the other line arguments)."""
    return _check_constraints(kw.get("prefix"), n, kw.get("line_lengths"), kw.get("line_end_ids"), rows, length, sh, "%d rows" % rows,
                              kw.get("templates"), kw.get("rhyme_scheme"), kw.get("rhyme_classes"), kw.get("rhyme_distinct", False), scheme).lines


# ------------------------------------------------------------------ 1. kernels
SRC = [[-1, 0, 0]] * 4 + [[-1, 0, -1], [-1, 0, 0], [-1, -1, 0], [-1, -1, -1]]      # "AAA" x 4, "AA", "AAA", "A.A", no scheme


def _copy_from(b, j, held):
    """The lyric index row b copies into index j under SRC (None: j is no copy column of the row)."""
    l, q = j // SENT, j % SENT
    if held or q in (0, SENT - 1) or l >= 3 or SRC[b][l] < 0:
        return None
    return j - (l - SRC[b][l]) * SENT


@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("templates", [False, True])
@pytest.mark.parametrize("distinct", [False, True])
def test_refrain_entries_copy_on_copy_columns_and_are_the_rhyme_entries_elsewhere(n, templates, distinct):
    """test_rhyme_gpu._kernel_case's inputs (8 rows, its V, random logits and histories, bounds / templates / rhyme tables on every
    line -- copy lines included: the copy comes before all of them) under the table SRC.  On a copy column select, sample and the
    candidates give the source's id, the candidates as (0, id) then -inf; on every other column, row by row, what the *_rhyme entries
    give on the same inputs, bit for bit.  Without logits the select entry writes the copies and leaves the other rows as the plain
    launch without logits leaves them; a null src fails before any launch."""
    B, P, V, Vp, Tmax, length, logits, uni, seq0, tabs, lens, tm = _kernel_case(n, distinct, templates)
    nb, uni, lg = 4, uni.to(DEV), logits.to(DEV)
    dt, dr = device_tables(tabs), device_rhyme(tabs)
    tmd = None if tabs.tmpl is None else torch.from_numpy(tabs.tmpl).to(DEV)
    src = torch.tensor(SRC, dtype=torch.int8, device=DEV)
    seq0[4, P + 39] = 4                                                        # content in front of the column at which row 4's source is PAD
    seq0[0, P + 1:P + SENT - 1] = torch.tensor([3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4])      # a full source line
    kinds = {"first": 0, "middle": 0, "last": 0, "pad_source": 0, "after_pad": 0, "cadence": 0, "held": 0, "free": 0, "differs": 0}
    for pos in (P, P + 7, P + 20, P + 21, P + 22, P + 29, P + 39, P + 41, P + 42, P + 43, P + 44, P + 50, P + 57):
        j = pos + 1 - P
        s0 = seq0.clone()
        s0[5, P + j - 1] = 0                                                   # a row whose previous token is PAD
        host = s0[:, P:].tolist()
        s0 = s0.to(DEV)
        for fe in (None, torch.tensor([0, pos + 2, 0, pos + 1, 0, 0, pos + 5, 0], dtype=torch.int32, device=DEV)):
            held = [fe is not None and pos + 1 < int(fe[b]) for b in range(B)]
            frm = [_copy_from(b, j, held[b]) for b in range(B)]
            for b in range(B):
                if j % SENT in (0, SENT - 1):
                    kinds["cadence"] += 1
                elif held[b]:
                    kinds["held"] += 1
                elif frm[b] is None:
                    kinds["free"] += 1
                else:
                    kinds[{1: "first", SENT - 2: "last"}.get(j % SENT, "middle")] += 1
                    kinds["pad_source"] += host[b][frm[b]] == 0 and host[b][j - 1] not in (0, 1)
                    kinds["after_pad"] += host[b][frm[b]] != 0 and host[b][j - 1] == 0
            rows = [b for b in range(B) if frm[b] is not None]
            want = torch.tensor([host[b][frm[b]] for b in rows], dtype=torch.long, device=DEV)
            for kind in ("select", "sample"):
                a, b_ = s0.clone(), s0.clone()
                pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                if kind == "select":
                    hip.decode_select_rhyme(lg, Vp, V, a, pa[0:1], P, SENT, T, REP, B, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe, pos_next=pa[1:2])
                    hip.decode_select_refrain(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, B, src, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe,
                                              pos_next=pb[1:2])
                else:
                    hip.decode_sample_rhyme(lg, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe,
                                            pos_next=pa[1:2])
                    hip.decode_sample_refrain(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, 10, 0.7, uni, B, src, dt, dr, tmpl=tmd, ngram=n,
                                              fixed_end=fe, pos_next=pb[1:2])
                torch.cuda.synchronize()
                assert int(pb[1]) == pos + 1 == int(pa[1])
                assert torch.equal(b_[rows, pos + 1], want), (pos, kind, fe is None, rows, b_[rows, pos + 1].tolist(), want.tolist())
                if rows:
                    kinds["differs"] += int((a[rows, pos + 1] != want).sum())
                    a[rows, pos + 1] = want                                    # every other row, and every other column of these
                assert torch.equal(a, b_), (pos, kind, fe is None, a[:, pos + 1].tolist(), b_[:, pos + 1].tolist())
            cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
            cvb, cib = cva.clone(), cia.clone()
            pp = torch.tensor([pos], dtype=torch.int32, device=DEV)
            hip.decode_beam_candidates_rhyme(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe)
            hip.decode_beam_candidates_refrain(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cvb, cib, B, src, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe)
            torch.cuda.synchronize()
            if rows and j % SENT not in (0, SENT - 1):
                assert cvb[rows].tolist() == [[0.0] + [NEG] * (nb - 1)] * len(rows), (pos, fe is None)
                assert cib[rows].tolist() == [[int(v)] + [0] * (nb - 1) for v in want.tolist()], (pos, fe is None)
                cva[rows], cia[rows] = cvb[rows], cib[rows]
            assert torch.equal(cva.view(torch.int32), cvb.view(torch.int32)) and torch.equal(cia, cib), (pos, fe is None)      # raw bits
            # without logits: the copies, the cadence, and nothing else
            a, b_ = s0.clone(), s0.clone()
            pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
            pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
            hip._select("" if fe is None else "_fixed", None, 0, 0, a, pa[0:1], P, SENT, T, REP, B, pa[1:2], fixed_end=fe)
            hip.decode_select_refrain(None, 0, V, b_, pb[0:1], P, SENT, T, REP, B, src, dt, dr, tmpl=tmd, ngram=n, fixed_end=fe, pos_next=pb[1:2])
            torch.cuda.synchronize()
            assert int(pb[1]) == pos + 1 == int(pa[1])
            assert torch.equal(b_[rows, pos + 1], want), (pos, fe is None)
            if rows:
                a[rows, pos + 1] = want
            assert torch.equal(a, b_), (pos, fe is None)
    # every kind of column the rule distinguishes was among them, and the copies are not what the other rules would have written
    assert min(kinds.values()) > 0, kinds
    # a null src: an error code, and no launch (nothing written, the position not published)
    b_ = s0.clone()
    pb = torch.tensor([P + 22, -1], dtype=torch.int32, device=DEV)
    for call in (lambda: hip.decode_select_refrain(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, B, None, dt, dr, tmpl=tmd, ngram=n, pos_next=pb[1:2]),
                 lambda: hip.decode_select_refrain(None, 0, V, b_, pb[0:1], P, SENT, T, REP, B, None, dt, dr, tmpl=tmd, ngram=n, pos_next=pb[1:2]),
                 lambda: hip.decode_sample_refrain(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, 10, 0.7, uni, B, None, dt, dr, tmpl=tmd, ngram=n,
                                                   pos_next=pb[1:2]),
                 lambda: hip.decode_beam_candidates_refrain(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, nb, cvb, cib, B, None, dt, dr, tmpl=tmd,
                                                            ngram=n)):
        with pytest.raises(RuntimeError, match="src \\[B, n_lines\\] is needed"):
            call()
    torch.cuda.synchronize()
    assert torch.equal(b_, s0) and int(pb[1]) == -1


# ------------------------------------------------------------------ 2. a scheme that asks nothing
def test_a_scheme_of_dots_through_the_refrain_entries_is_the_rhyme_entries():
    """src all -1: every column is the *_rhyme entries', with their tables; and with the "no rule" forms of the tables (no line
    tables at all, n_lines the width of src) the *_lines entries' under unconstrained bounds."""
    B, P, V, Vp, Tmax, length, logits, uni, seq0, tabs, lens, tm = _kernel_case(0, True, True)
    nb, uni, lg, seq0 = 4, uni.to(DEV), logits.to(DEV), seq0.to(DEV)
    dt, dr = device_tables(tabs), device_rhyme(tabs)
    tmd = torch.from_numpy(tabs.tmpl).to(DEV)
    src = torch.full((B, 3), -1, dtype=torch.int8, device=DEV)
    free = device_tables(check_lines((0, CAP), None, B, length, SENT, V))
    for n in (0, 3):
        for pos in (P, P + 1, P + 7, P + 9, P + 20, P + 21, P + 24, P + 27, P + 30, P + 47):
            for tables, rh, t_, ref in ((dt, dr, tmd, "rhyme"), (None, None, None, "lines")):
                a, b_, c_, d_ = (seq0.clone() for _ in range(4))
                pp = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
                cvb, cib = cva.clone(), cia.clone()
                if ref == "rhyme":
                    hip.decode_select_rhyme(lg, Vp, V, a, pp[0:1], P, SENT, T, REP, B, dt, dr, tmpl=tmd, ngram=n, pos_next=pp[1:2])
                    hip.decode_sample_rhyme(lg, Vp, V, c_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, dr, tmpl=tmd, ngram=n, pos_next=pp[1:2])
                    hip.decode_beam_candidates_rhyme(lg, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cva, cia, B, dt, dr, tmpl=tmd, ngram=n)
                else:
                    hip.decode_select_lines(lg, Vp, V, a, pp[0:1], P, SENT, T, REP, B, free, ngram=n, pos_next=pp[1:2])
                    hip.decode_sample_lines(lg, Vp, V, c_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, free, ngram=n, pos_next=pp[1:2])
                    hip.decode_beam_candidates_lines(lg, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cva, cia, B, free, ngram=n)
                hip.decode_select_refrain(lg, Vp, V, b_, pp[0:1], P, SENT, T, REP, B, src, tables, rh, tmpl=t_, ngram=n, pos_next=pp[1:2])
                hip.decode_sample_refrain(lg, Vp, V, d_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, src, tables, rh, tmpl=t_, ngram=n,
                                          pos_next=pp[1:2])
                hip.decode_beam_candidates_refrain(lg, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cvb, cib, B, src, tables, rh, tmpl=t_, ngram=n)
                torch.cuda.synchronize()
                assert torch.equal(a, b_) and torch.equal(c_, d_), (ref, n, pos)
                assert torch.equal(cva.view(torch.int32), cvb.view(torch.int32)) and torch.equal(cia, cib), (ref, n, pos)


# ------------------------------------------------------------------ 3. the decoders on their own output
def _holds(ids, tabs, n, row_of=lambda b: b, rows=None):
    """Every copy column of every row of ids repeats its source's, and no other column breaks the n-gram rule given the full history."""
    total = 0
    for b, r in enumerate(ids.cpu().tolist()):
        total += copies_hold(r, tabs, row_of(b))
        assert ngram_violations(r, tabs, row_of(b), n) == [], b
    return total


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_decoders_repeat_line_0_as_line_3_under_ngram_blocking(mode):
    """Under "AB.A" with no_repeat_ngram_size=3 -- which alone forbids a line to come back --, on the GPU's own output: line 3 is
    line 0 column by column in every row; every id before the copy line is the id of the run without the argument (the rule never
    touches a free column); no other column breaks the n-gram rule given the full history, copied text included.  Greedy, sampling
    with the same uniforms, four beams and eight beams in four groups (every returned beam), and one beam is greedy."""
    model, tb = build("tiny_s5", mode)
    sh = setup_case("tiny_s5")[1]
    n, scheme, first = 3, "AB.A", 3 * SENT + 1
    tabs = refrain_tables(sh, 3, LENGTH, scheme, n)
    args = dict(temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n)
    dec = GreedyDecoder(model, 3, max_len=LENGTH)
    plain = dec.generate(tb, LENGTH, **args)
    greedy = dec.generate(tb, LENGTH, refrain_scheme=scheme, **args)
    assert dec.rules.refrain is not None and dec.rules.lines is None and any("refrain" in k for k in dec.graphs)
    assert _holds(greedy, tabs, n) == 3 * CAP and torch.equal(greedy[:, :first], plain[:, :first])
    assert all(lines_of(r)[3] == lines_of(r)[0] and any(lines_of(r)[0]) for r in greedy.cpu().tolist())
    assert not all(lines_of(r)[3] == lines_of(r)[0] for r in plain.cpu().tolist())              # blocking alone: the line cannot come back
    gen = lambda: torch.Generator(device=DEV).manual_seed(17)                  # noqa: E731
    splain = dec.generate(tb, LENGTH, top_k=10, top_p=0.7, generator=gen(), **args)
    sampled = dec.generate(tb, LENGTH, top_k=10, top_p=0.7, generator=gen(), refrain_scheme=scheme, **args)
    assert _holds(sampled, tabs, n) == 3 * CAP and torch.equal(sampled[:, :first], splain[:, :first])
    assert not torch.equal(sampled, greedy)
    one, _ = BeamDecoder(model, 3, 1, max_len=LENGTH).generate(tb, LENGTH, refrain_scheme=scheme, **args)
    assert torch.equal(one[:, 0], greedy)
    for nb, groups in ((4, {}), (8, dict(num_beam_groups=4, diversity_penalty=0.5))):
        bd = BeamDecoder(model, 3, nb, max_len=LENGTH)
        ids, scores = bd.generate(tb, LENGTH, refrain_scheme=scheme, **args, **groups)
        assert torch.isfinite(scores).all()
        assert _holds(ids.reshape(3 * nb, -1), tabs, n, row_of=lambda r: r // nb) == 3 * nb * CAP
        # the beams as they stand when the copy line ends are the beams of the run without the argument when it starts: a copy
        # keeps every beam and its score, and a run that goes on reorders them, so the two are compared where nothing has yet
        cut, _ = bd.generate(tb, 3 * SENT, **args, **groups)
        upto, sc = bd.generate(tb, 4 * SENT - 1, refrain_scheme=scheme, **args, **groups)
        assert torch.equal(upto[:, :, :first], cut) and torch.equal(sc, _)
        assert _holds(upto.reshape(3 * nb, -1), refrain_tables(sh, 3, 4 * SENT - 1, scheme, n), n, row_of=lambda r: r // nb) == 3 * nb * CAP


# ------------------------------------------------------------------ 4. greedy against the CPU restatement
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_greedy_under_a_scheme_is_the_cpu_restatement(mode):
    """The copy is line 1 ("AAB.B"; row 2's line 2 ends early, so its copy repeats PADs), and the restatement's arg-max margins carry
    the comparison past that line's end in every fixture row (test_refrain_cpu holds them to that on the CPU)."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    dec = GreedyDecoder(model, 3, max_len=LENGTH)
    for scheme, n in (("AAB.B", 0), ("AAB.B", 3), ("AA...", 3)):
        tabs = refrain_tables(sh, 3, LENGTH, scheme, n)
        ids = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, refrain_scheme=scheme).cpu()
        for row in range(3):
            want, gaps = cpu_refrain_greedy(w, sh, table, start_row(batch, row), LENGTH, tabs, b=row, n=n)
            upto = comparable_length(gaps, LENGTH)
            assert upto > 2 * SENT - 1, (scheme, n, row, upto)                 # past the copy line's end: the comparison is not vacuous
            assert ids[row, :1 + upto].tolist() == want[:1 + upto], (scheme, n, row)
            assert copies_hold(ids[row].tolist(), tabs, row) == CAP * (2 if scheme == "AAB.B" else 1)
    assert dec.skipped_steps == CAP


# ------------------------------------------------------------------ 5. head skipping
def test_skipping_the_head_on_copy_columns_changes_no_id(monkeypatch):
    model, tb = build("tiny_s5", "bf16")
    n, scheme = 3, "AB.AA"
    runs = {}
    for skip in ("1", "0"):
        monkeypatch.setenv("MMTG_DECODE_REFRAIN_SKIP", skip)
        dec = GreedyDecoder(model, 3, max_len=LENGTH)
        heads = []
        tap = lambda j, with_head, picked, logits: heads.append(with_head)      # noqa: E731
        greedy = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, refrain_scheme=scheme, tap=tap)
        g_skipped, g_heads = dec.skipped_steps, sum(heads)
        sampled = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, no_repeat_ngram_size=n,
                               generator=torch.Generator(device=DEV).manual_seed(29), refrain_scheme=scheme)
        eager = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, refrain_scheme=scheme, use_graph=False)
        assert torch.equal(eager, greedy)
        runs[skip] = (greedy, sampled, g_skipped, dec.skipped_steps, g_heads, set(dec.graphs))
    on, off = runs["1"], runs["0"]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and not torch.equal(on[0], on[1])
    assert on[2] == 2 * CAP == on[3] and off[2] == 0 == off[3]                 # two copy lines, every row copies on them
    assert off[4] - on[4] == 2 * CAP                                           # as many steps fewer called the head
    assert any(not k[0] and "refrain" in k for k in on[5]) and not any(not k[0] and "refrain" in k for k in off[5])
    # per-prompt schemes: a column skips only where EVERY row copies; return_logprobs keeps the head everywhere
    monkeypatch.delenv("MMTG_DECODE_REFRAIN_SKIP")
    dec = GreedyDecoder(model, 3, max_len=LENGTH)
    mixed = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, refrain_scheme=["AB.AA", "AB.A", None])
    assert dec.skipped_steps == 0
    sh = setup_case("tiny_s5")[1]
    assert _holds(mixed, refrain_tables(sh, 3, LENGTH, ["AB.AA", "AB.A", None]), 0) == 3 * CAP
    two = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, refrain_scheme=["AB.AA", "AB.A", "A..A"])
    assert dec.skipped_steps == CAP and _holds(two, refrain_tables(sh, 3, LENGTH, ["AB.AA", "AB.A", "A..A"]), 0) == 4 * CAP
    ids, lp = dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, refrain_scheme=scheme, return_logprobs=True)
    assert dec.skipped_steps == 0 and torch.equal(ids, dec.generate(tb, LENGTH, temperature=T, repitition_penalty=REP, refrain_scheme=scheme))


# ------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_schemes_compose_with_a_partial_prefix_bounds_a_template_a_rhyme_scheme_and_logprobs(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    cid = content_ids(fx)
    classes, _ = fixture_rhymes(fx)
    length = 4 * SENT
    pre = [[1, cid[22], cid[23]], [1], _line_of(cid[20], cid[21], cid[5]) + [1]]           # partial source line; none; a whole given source
    tm = [[(cid[22], None, Ellipsis)], None, None]                             # row 0's source line is templated
    lens = [[(3, 8), (3, 8), (2, 6), (3, 8)], [(3, 8), (3, 8), (2, 6)], [None, (3, 8), (3, 8)]]       # the source's bounds, or none, on line 3
    kw = dict(line_lengths=lens, templates=tm, rhyme_scheme=["XX..", ".XX.", ".XX."], rhyme_classes=classes, prefix=pre)
    scheme = ["AB.A", "A..A", "A..A"]
    tabs = refrain_tables(sh, 3, length, scheme, **kw)
    assert not tabs.bare and tabs.src[:, 3].tolist() == [0, 0, 0]
    dec = GreedyDecoder(model, 3, max_len=length)
    ids, lp = dec.generate(tb, length, temperature=T, repitition_penalty=REP, refrain_scheme=scheme, return_logprobs=True, **kw)
    assert dec.skipped_steps == 0 and dec.rules.lines is not None and dec.rules.tmpl is not None and dec.rules.rhyme is not None
    rows = ids.cpu().tolist()
    for b, p in enumerate(pre):
        assert rows[b][:len(p)] == p
        assert copies_hold(rows[b], tabs, b, start=len(p)) == CAP and lines_of(rows[b])[3] == lines_of(rows[b])[0]
        assert rhyme_violations(rows[b], tabs, b, start=len(p)) == [], b       # bounds, the template, the rhymes: on every line
        assert all(ok for _, _, ok in followers_rhyme(rows[b], tabs, b))
    assert rows[0][1:3] == [cid[22], cid[23]] and rows[2][1:4] == [cid[20], cid[21], cid[5]] and rows[2][3 * SENT + 1:3 * SENT + 4] == rows[2][1:4]
    assert sum(len(followers_rhyme(r, tabs, b)) for b, r in enumerate(rows)) >= 2
    assert all(3 <= sum(v != 0 for v in lines_of(r)[3]) for r in rows[:2])
    same = dec.generate(tb, length, temperature=T, repitition_penalty=REP, refrain_scheme=scheme, **kw)          # skipping the head
    assert torch.equal(same, ids) and dec.skipped_steps == CAP
    # the log-probability node scores whatever the column holds: a copied id at the model's log-probability of it
    lp = lp.cpu().numpy()
    got = score_sequences(model, {k: v.cpu().numpy() for k, v in tb.items()}, ids)
    copy = [j for j in range(3 * SENT + 1, 3 * SENT + 1 + CAP)]
    assert np.isfinite(lp[:, copy]).all() and (lp[:, copy] < 0).all()
    diff = np.abs(got[:, copy].astype(np.float64) - lp[:, copy]).max()
    print("%s: tok_lp on copy columns against score_sequences, max |difference| %.3g (bound %.3g)" % (mode, diff, PARITY[mode]))
    assert diff <= PARITY[mode]
    bids, sc = BeamDecoder(model, 3, 4, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, refrain_scheme=scheme, **kw)
    flat = bids.reshape(12, -1).cpu().tolist()
    for r in range(12):
        p = pre[r // 4]
        assert flat[r][:len(p)] == p and copies_hold(flat[r], tabs, r // 4, start=len(p)) == CAP
        assert rhyme_violations(flat[r], tabs, r // 4, start=len(p)) == [], r
    assert torch.isfinite(sc).all()


def _line_of(*content):
    return [1] + list(content) + [0] * (CAP - len(content)) + [2]


# ------------------------------------------------------------------ 7. off means off
def test_refrain_scheme_none_is_exactly_the_call_without_the_argument(monkeypatch):
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
    for kw in (dict(), dict(refrain_scheme=None)):
        del names[:]
        dec = GreedyDecoder(model, 3, use_graph=False)
        ids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)
        sids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                            generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        bids, sc = BeamDecoder(model, 3, 4, use_graph=False).generate(tb, 220, temperature=T, repitition_penalty=REP, **kw)
        runs.append((list(names), ids, sids, bids, sc))
        assert dec.rules.refrain is None and dec.rules.rhyme is None and dec.rules.tmpl is None and dec.rules.lines is None and dec.copy_cols is None
        assert dec.skipped_steps == 0
    assert runs[0][0] == runs[1][0] and not any("_refrain" in x or "_rhyme" in x or "_lines" in x for x in runs[0][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    del names[:]
    GreedyDecoder(model, 3, use_graph=False).generate(tb, 220, temperature=T, repitition_penalty=REP, refrain_scheme="AB.A")
    BeamDecoder(model, 3, 4, use_graph=False).generate(tb, 220, temperature=T, repitition_penalty=REP, refrain_scheme="AB.A")
    assert set(names) == {"mmtg_decode_select", "mmtg_decode_select_refrain", "mmtg_decode_beam_candidates_refrain", "mmtg_decode_beam_merge"}
    monkeypatch.undo()
    fresh, dec = GreedyDecoder(model, 3), GreedyDecoder(model, 3)
    a = fresh.generate(tb, 220, temperature=T, repitition_penalty=REP)
    b = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, refrain_scheme=None)
    assert torch.equal(a, b) and torch.equal(a, runs[0][1]) and set(dec.graphs) == set(fresh.graphs)
    keys = set(dec.graphs)
    c = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, refrain_scheme="..........")       # the *_refrain entries, nothing asked
    assert torch.equal(a, c) and dec.rules.refrain is not None and dec.copy_cols is None and dec.skipped_steps == 0
    new = set(dec.graphs) - keys
    assert new and all("refrain" in k and k[0] for k in new)                   # head steps only; the others replay the graphs they had
    d = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, refrain_scheme="AA")
    assert not torch.equal(a, d) and dec.skipped_steps == CAP
    assert torch.equal(dec.generate(tb, 220, temperature=T, repitition_penalty=REP), a) and dec.rules.refrain is None and dec.rules.lines is None


# ------------------------------------------------------------------ 8. full size
def test_full_size_bf16_under_a_scheme_is_bit_stable_and_repeats_its_lines():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    B, Ln, n = 256, 220, 3
    nbt = synth.make_batch(B, mcfg, dcfg, V, seed=13)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    scheme = "AB.AB.AB.A"
    dec = GreedyDecoder(model, B, max_len=Ln, lanes=1)
    assert dec.fused and dec.use_graph
    sh = dec.eng.sh
    tabs = refrain_tables(sh, B, Ln, scheme, n)
    args = dict(temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, refrain_scheme=scheme)
    g1 = dec.generate(batch, Ln, **args)
    assert dec.skipped_steps == 5 * CAP                                        # lines 3, 4, 6, 7 and 9 are copies
    assert torch.equal(dec.generate(batch, Ln, **args), g1)
    assert _holds(g1[:32], tabs, n) == 32 * 5 * CAP
    src = torch.from_numpy(tabs.src[0].astype(np.int64))
    body = g1[:, 1:].reshape(B, 10, SENT)[:, :, :CAP]                          # [B, line, content column]
    for l in range(10):
        if src[l] >= 0:
            assert torch.equal(body[:, l], body[:, int(src[l])]), l
    assert int(g1.min()) >= 0 and int(g1.max()) < V and (body[:, 0] != 0).any()
    s1 = dec.generate(batch, Ln, top_k=10, top_p=0.7, generator=torch.Generator(device=DEV).manual_seed(21), **args)
    assert torch.equal(dec.generate(batch, Ln, top_k=10, top_p=0.7, generator=torch.Generator(device=DEV).manual_seed(21), **args), s1)
    sb = s1[:, 1:].reshape(B, 10, SENT)[:, :, :CAP]
    assert all(torch.equal(sb[:, l], sb[:, int(src[l])]) for l in range(10) if src[l] >= 0) and not torch.equal(s1, g1)


# ------------------------------------------------------------------ 9. lanes
@pytest.mark.parametrize("use_graph", [True, False])
def test_two_lanes_read_their_own_rows_of_every_table(use_graph):
    """Four rows whose prefix lengths, bounds, templates, rhyme and refrain schemes all differ between rows 0-1 and rows 2-3, under
    no_repeat_ngram_size=3 and a min_p draw: a decoder of two lanes gives every row a view of its own rows of each table (and of the
    uniforms), so its ids are those of the one-lane decoder bit for bit, replayed and eager.  Three lines: the third carries the
    copies."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", "bf16")
    tb4 = {k: torch.cat([v, v[:1]], 0) for k, v in tb.items()}
    cid = content_ids(fx)
    classes, _ = fixture_rhymes(fx)
    length = 3 * SENT
    pre = [[1], [1, cid[22], cid[23]], [1, cid[20]], [1, cid[21], cid[5], cid[22], cid[23]]]
    kw = dict(temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0, min_p=0.05, prefix=pre, no_repeat_ngram_size=3,
              line_lengths=[[(3, 8), (3, 8), (3, 8)], [(2, 6), (3, 8), None], [(3, 8), (2, 9), (3, 8)], [(4, 7), (3, 8), (3, 8)]],
              line_end_ids=[None, [None, [cid[7], cid[8], cid[9]], None], None, None],
              templates=[None, [None, (cid[5], Ellipsis)], [None, (cid[22], None, Ellipsis)], None],
              rhyme_scheme=["AA", "A.A", "AA", "AA"], rhyme_classes=classes, refrain_scheme=["A.A", None, "A.A", ".AA"])
    tabs = refrain_tables(sh, 4, length, kw["refrain_scheme"], 3, **{k: kw[k] for k in ("prefix", "line_lengths", "line_end_ids", "templates",
                                                                                       "rhyme_scheme", "rhyme_classes")})
    for t in (tabs.lo, tabs.hi, tabs.set_of, tabs.tmpl, tabs.lead, tabs.src):   # (rows 2-3 are not rows 0-1 in any table)
        assert not np.array_equal(t[:2], t[2:])
    gen = lambda: torch.Generator(device=DEV).manual_seed(17)                    # noqa: E731
    one = GreedyDecoder(model, 4, max_len=length, lanes=1, use_graph=use_graph)
    two = GreedyDecoder(model, 4, max_len=length, lanes=2, use_graph=use_graph)
    a = one.generate(tb4, length, generator=gen(), **kw)
    b = two.generate(tb4, length, generator=gen(), **kw)
    assert torch.equal(a, b), (a.tolist(), b.tolist())
    assert bool(two.graphs) == use_graph and len(two.children) == 2
    rows = a.cpu().tolist()
    for r, p in enumerate(pre):
        assert rows[r][:len(p)] == p and rhyme_violations(rows[r], tabs, r, start=len(p)) == [], r
    assert lines_of(rows[0])[2] == lines_of(rows[0])[0] and lines_of(rows[3])[2] == lines_of(rows[3])[1]
    assert not torch.equal(a[0], a[3])                                          # (the same prompt under other rules and draws)
