"""Keyword-constrained beam search on the MI355X (BeamDecoder with keywords=): the candidates kernel and the merge kernel against
the host restatements of tests/test_keywords_cpu.py, all banks equal against the plain merge, the decoder against the CPU search,
and the surfaces above it (return_met, prefixes, the other constraints, generate_beams)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import keyword_bank, keyword_met_mask, keyword_select, keywords_met  # noqa: E402
from mmtg_amd.decode import BeamDecoder  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case  # noqa: E402
from test_beam_gpu import build, rescore  # noqa: E402
from test_keywords_cpu import CASE, FULL, KEYWORDS, NB, REP, ROW, T, cpu_keyword_run, keyword_candidates  # noqa: E402
from test_lines_cpu import CAP  # noqa: E402
from test_ngram_cpu import banned_ids, repeated_ngrams, violations  # noqa: E402

DEV = "cuda"
NEG = np.float32(-np.inf)
P, TMAX, POS = 5, 48, 37


# ------------------------------------------------------------------ 6. the candidates kernel
@pytest.mark.parametrize("V,Vp", [(13317, 13320), (160, 168)])
def test_keyword_candidates_are_the_host_restatement(V, Vp):
    """3 prompts x 4 beams, K = 3 phrases of 1, 2 and 4 ids, every row about to fill column 9 of line 2 (j = 54), under the rhyme
    form with unconstrained bounds, no_repeat_ngram_size = 2 and a template table: one hand-built history per case."""
    nb, n, K, Tm, ng = 4, 3, 3, 80, 2
    B, W, j = n * nb, nb + K, 2 * SENT + 10
    pos = P + j - 1
    top = V - 1
    a, b1, b2, c1, c2, c3, c4 = top - 1, top - 2, top - 3, top - 4, top - 5, top - 6, top - 7
    x_, y_ = top - 8, top - 9
    # prompts 0 and 2: three distinct first ids; prompt 1: the two longer phrases both start with b1 (the second slot is dead)
    lists = [[(a,), (b1, b2), (c1, c2, c3, c4)], [(a,), (b1, b2), (b1, c2, c3, c4)], [(a,), (b1, b2), (c1, c2, c3, c4)]]
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(B, Vp, generator=g) * 3
    seq = torch.randint(3, min(V, 99), (B, Tm), generator=g)
    seq[seq == 2] = 3
    for s in range(0, Tm - P, SENT):                                 # the cadence of the history
        seq[:, P + s] = 1
        if s + SENT - 1 < Tm - P:
            seq[:, P + s + SENT - 1] = 2
    gen = seq[:, P:]
    gen[0, 5:7] = torch.tensor([b1, b2])                             # row 0: (b1, b2) met in line 0 ...
    gen[0, SENT + 3] = a                                             # ... and (a,) in line 1
    gen[1, j - 1] = c1                                               # row 1: progress 1 of the four-phrase
    gen[2, j - 3:j] = torch.tensor([c1, c2, c3])                     # row 2: progress 3
    gen[3, j - 3:j] = torch.tensor([c1, c2, x_])                     # row 3: a broken progress
    gen[4, 7:9] = torch.tensor([y_, b1])                             # row 4: (y, b1) is held and the history ends in y: b1, the next id
    gen[4, j - 1] = y_                                               # of the unmet (b1, b2) and (b1, c2, c3, c4), is banned
    logits[5, a] = 50.0                                              # row 5: a is the row's best id (its keyword slot is dead)
    gen[6, j - 1] = b1                                               # row 6: progress 1 of both phrases that start with b1
    gen[7, j - 2:j] = 0                                              # row 7: sticky PAD
    gen[8, j - 1] = b1                                               # row 8: a template gives b2 at this column, which completes (b1, b2)
    gen[9, SENT + 2:SENT + 6] = torch.tensor([c1, c2, c3, c4])       # row 9: the four-phrase met in line 1, progress 1 of (b1, b2)
    gen[9, j - 1] = b1
    gen[10, SENT - 3:SENT + 2] = torch.tensor([c1, c2, 2, 1, c3])    # row 10: a phrase cut by the cadence is not met
    phrases = torch.full((n, 8, 4), -1, dtype=torch.int32)
    lens = torch.zeros(n, 8, dtype=torch.int8)
    for p_, row in enumerate(lists):
        for i, ph in enumerate(row):
            phrases[p_, i, :len(ph)] = torch.tensor(ph, dtype=torch.int32)
            lens[p_, i] = len(ph)
    n_lines = 3
    lo, hi = torch.zeros(B, n_lines, dtype=torch.uint8), torch.full((B, n_lines), CAP, dtype=torch.uint8)
    sets = torch.zeros(1, (V + 31) // 32, dtype=torch.int32)
    set_of = torch.full((B, n_lines), -1, dtype=torch.int16)
    tmpl = torch.full((B, n_lines, CAP), -1, dtype=torch.int32)
    tmpl[8, 2, 9] = b2
    class_of, lead = torch.full((V,), -1, dtype=torch.int16), torch.full((B, n_lines), -1, dtype=torch.int8)
    d = lambda t: t.to(DEV)                                          # noqa: E731
    tables, rhyme = (d(lo), d(hi), d(sets), d(set_of)), (d(class_of), d(lead), False)
    dl, ds, posd = d(logits), d(seq), torch.tensor([pos], dtype=torch.int32, device=DEV)
    cv, ci, cb = torch.full((B, W), 7.0, device=DEV), torch.full((B, W), -7, dtype=torch.int32, device=DEV), torch.full((B, W), -7, dtype=torch.int32, device=DEV)
    hip.decode_beam_candidates_kw(dl, Vp, V, ds, posd, P, SENT, T, REP, nb, cv, ci, cb, B, (d(phrases), d(lens), K, 4), tables=tables,
                                  rhyme=rhyme, tmpl=d(tmpl), ngram=ng)
    rv, ri = torch.zeros(B, nb, device=DEV), torch.zeros(B, nb, dtype=torch.int32, device=DEV)
    hip.decode_beam_candidates_rhyme(dl, Vp, V, ds, posd, P, SENT, T, REP, nb, rv, ri, B, tables, rhyme, tmpl=d(tmpl), ngram=ng)
    torch.cuda.synchronize()
    cv, ci, cb, rv, ri = cv.cpu(), ci.cpu(), cb.cpu(), rv.cpu(), ri.cpu()
    # slots 0 .. nb - 1 are the rhyme form's, bit for bit
    assert cv[:, :nb].numpy().tobytes() == rv.numpy().tobytes() and torch.equal(ci[:, :nb], ri)
    for b in range(B):
        hist, ph = gen[b, :j].tolist(), lists[b // nb]
        if b == 7 or b == 8:                                          # one candidate: PAD / the given id, the score unchanged
            tok = 0 if b == 7 else b2
            want = [(np.float32(0.0), keyword_bank(hist + [tok], ph), tok)] + [(NEG, 0, 0)] * (W - 1)
        else:
            x = O.process_logits(logits[b], torch.tensor(hist), T, REP)[:V]
            for v in banned_ids(hist, ng):
                x[v] = float("-inf")
            want = keyword_candidates(x, hist, np.float32(0.0), nb, ph, V)
        assert ci[b].tolist() == [c[2] for c in want], b
        assert cb[b].tolist() == [c[1] for c in want], b
        wv = np.array([c[0] for c in want], np.float32)
        assert np.array_equal(np.isinf(cv[b].numpy()), np.isinf(wv)), b
        np.testing.assert_allclose(cv[b].numpy(), wv, rtol=1e-6, atol=1e-6)
    # the cases bite
    dead = lambda b, i: ci[b, nb + i] == 0 and cv[b, nb + i] == NEG and cb[b, nb + i] == 0           # noqa: E731
    assert dead(0, 0) and dead(0, 1) and not dead(0, 2) and cb[0, nb + 2] == 3 + 1                  # met: 1 + 2; the slot starts c1
    assert ci[1, nb + 2] == c2 and cb[1, nb + 2] == 2 and ci[2, nb + 2] == c4 and cb[2, nb + 2] == 4
    assert ci[3, nb + 2] == c1 and cb[3, nb + 2] == 1                                               # broken: from the start again
    h4 = gen[4, :j].tolist()                                          # the ban wins: unmet keywords, their next id banned, dead slots
    assert keyword_met_mask(h4, lists[1]) == [False, False, False] and b1 in banned_ids(h4, ng) and a not in banned_ids(h4, ng)
    assert dead(4, 1) and dead(4, 2) and ci[4, nb + 0] == a and b1 not in ci[4].tolist()
    assert dead(5, 0) and ci[5, 0] == a and cb[5, 0] == 1
    assert ci[6, nb + 1] == b2 and cb[6, nb + 1] == 2 and ci[6, nb + 2] == c2 and cb[6, nb + 2] == 2
    assert ci[5, nb + 1] == b1 and dead(5, 2) and dead(7, 2)                                          # two keywords, one id: the second is dead
    assert ci[7].tolist() == [0] * W and cb[7].tolist() == [0] * W and cv[7, 0] == 0
    assert ci[8, 0] == b2 and cb[8, 0] == 2 and cv[8, 0] == 0 and cv[8, 1:].eq(NEG).all()
    assert dead(9, 2) and ci[9, nb + 1] == b2 and cb[9, nb + 1] == 4 + 2
    assert not dead(10, 2) and ci[10, nb + 2] == c1


# ------------------------------------------------------------------ 7. the merge kernel
def _tables(nb, K, n=3, seed=0, banks=True):
    """Host inputs of one merge over n prompts, as tests/test_groups_gpu.py builds them, nb + K candidates wide: -inf entries, one
    NaN, one dead parent, banks in 0 .. 6 (or all 0), random seq / keep / rows."""
    g = torch.Generator().manual_seed(1000 * nb + 10 * K + seed)
    B, W = n * nb, nb + K
    cv = -torch.rand(B, W, generator=g) * 3
    cv[torch.rand(B, W, generator=g) < 0.1] = float("-inf")
    cv[nb, 0] = float("nan")                                       # prompt 1, parent 0, slot 0
    ci = torch.randint(0, 140, (B, W), generator=g, dtype=torch.int32)
    cb = torch.randint(0, 7, (B, W), generator=g, dtype=torch.int32) if banks else torch.zeros(B, W, dtype=torch.int32)
    scores = -torch.rand(B, generator=g) * 2
    scores[2 * nb + nb - 1] = float("-inf")                        # prompt 2: its last parent is dead
    seq = torch.randint(3, 99, (B, TMAX), generator=g)
    keep = torch.randint(0, 2, (B, TMAX), generator=g, dtype=torch.int32)
    rows = torch.randint(0, B, (B, TMAX), generator=g, dtype=torch.int32)
    return cv, ci, cb, scores, seq, keep, rows


def _restate(cv, ci, cb, scores, seq, keep, rows, pos, nb, held=()):
    """The merge rule of include/mmtg_hip.h on host copies (keyword_select is the selection)."""
    out = [t.clone() for t in (scores, seq, keep, rows)]
    osc, oseq, okeep, orows = out
    cvn, scn, W = cv.numpy(), scores.numpy(), cv.shape[1]
    for b0 in range(0, seq.shape[0], nb):
        if b0 // nb in held:
            orows[b0:b0 + nb, pos + 1] = torch.arange(b0, b0 + nb, dtype=torch.int32)
            continue
        cands = [(np.float32(scn[b0 + p] + cvn[b0 + p, k]), int(cb[b0 + p, k]), int(ci[b0 + p, k])) for p in range(nb) for k in range(W)]
        for r, (o, sc, _, v) in enumerate(keyword_select(cands, nb)):
            b, src = b0 + r, b0 + o // W
            oseq[b, :pos + 1], okeep[b, :pos + 1], orows[b, :pos + 1] = seq[src, :pos + 1], keep[src, :pos + 1], rows[src, :pos + 1]
            oseq[b, pos + 1], orows[b, pos + 1], osc[b] = v, b, float(sc)
    return out


def _run(entry, cands, scores, seq, keep, rows, pos, nb, *tail, **kw):
    d = [None if t is None else t.to(DEV) for t in tuple(cands) + (scores, seq, keep, rows)]
    posd = torch.tensor([pos, -7], dtype=torch.int32, device=DEV)
    entry(*d, posd[0:1], P, SENT, nb, seq.shape[0] // nb, *tail, pos_next=posd[1:2], **kw)
    torch.cuda.synchronize()
    assert int(posd[1]) == pos + 1
    return [t.cpu() for t in d[-4:]]


def _same(got, want):
    return all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("nb,K", [(4, 3), (6, 2), (8, 8), (16, 0)])
def test_keyword_merge_is_the_host_restatement(nb, K):
    cv, ci, cb, scores, seq, keep, rows = _tables(nb, K)
    want = _restate(cv, ci, cb, scores, seq, keep, rows, POS, nb)
    got = _run(hip.decode_beam_merge_kw, (cv, ci, cb), scores, seq, keep, rows, POS, nb, K)
    assert _same(got, want), (nb, K)
    if K:                                                           # the banks changed what the plain order would keep
        flat = _restate(cv, ci, torch.zeros_like(cb), scores, seq, keep, rows, POS, nb)
        assert not _same(want, flat)
    # the *_fixed entry: prompt 1 held, and left as the plain *_fixed merge leaves it; the others as above
    fe = torch.full((3 * nb,), P + 1, dtype=torch.int32)
    fe[nb:2 * nb] = POS + 2
    got = _run(hip.decode_beam_merge_kw_fixed, (cv, ci, cb), scores, seq, keep, rows, POS, nb, fe.to(DEV), K)
    assert _same(got, _restate(cv, ci, cb, scores, seq, keep, rows, POS, nb, held=(1,))), (nb, K)
    plain = _run(hip.decode_beam_merge_fixed, (cv[:, :nb].contiguous(), ci[:, :nb].contiguous()), scores, seq, keep, rows, POS, nb, fe.to(DEV))
    assert _same([t[nb:2 * nb] for t in got], [t[nb:2 * nb] for t in plain])


@pytest.mark.parametrize("nb", [1, 4, 16])
def test_with_all_banks_equal_the_keyword_merge_is_the_plain_merge_bit_for_bit(nb):
    cv, ci, cb, scores, seq, keep, rows = _tables(nb, 0, seed=1, banks=False)
    for pos in (POS, P + 20, P + 21):                               # a selection, a forced [#EOS#], a forced [#START#]
        want = _run(hip.decode_beam_merge, (cv, ci), scores, seq, keep, rows, pos, nb)
        assert _same(_run(hip.decode_beam_merge_kw, (cv, ci, cb), scores, seq, keep, rows, pos, nb, 0), want), pos
    want = _run(hip.decode_beam_merge, (None, None), scores, seq, keep, rows, POS, nb)          # a step without the head
    assert _same(_run(hip.decode_beam_merge_kw, (None, None, None), scores, seq, keep, rows, POS, nb, 0), want)
    if nb == 4:                                                     # and wider tables whose keyword slots are all dead
        wide = [torch.cat([t, f], 1) for t, f in ((cv, torch.full((3 * nb, 3), float("-inf"))), (ci, torch.zeros(3 * nb, 3, dtype=torch.int32)),
                                                 (cb, torch.zeros(3 * nb, 3, dtype=torch.int32)))]
        want = _run(hip.decode_beam_merge, (cv, ci), scores, seq, keep, rows, POS, nb)
        assert _same(_run(hip.decode_beam_merge_kw, wide, scores, seq, keep, rows, POS, nb, 3), want)


# ------------------------------------------------------------------ 8. the decoder follows the CPU search
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_four_beams_with_keywords_follow_the_cpu_search(mode):
    """The prompt and keywords of tests/test_keywords_cpu.py (the plain search holds neither keyword), compared over the generated
    positions before the CPU search's first selection with a gap below 1e-4 between two candidates of one bank that are adjacent in
    the bank's order, one of them ranked below nb: ids, order and met equal, scores within 1e-3; and every score re-scores."""
    gaps = cpu_keyword_run()[2]
    L = comparable_length(gaps, FULL)
    print("comparable run", L, "smallest in-bank gap before it", min(g for c, g in gaps if c <= L))
    assert L >= 2 * SENT
    cids, cscores, _, cmet = cpu_keyword_run(L)
    assert keywords_met(cids[0].tolist(), KEYWORDS) >= 1            # a keyword completes inside the compared run
    model, tb = build(CASE, mode)
    n = tb["img_embs"].shape[0]
    dec = BeamDecoder(model, n, NB, max_len=FULL)
    ids, scores, met = dec.generate(tb, L, temperature=T, repitition_penalty=REP, keywords=[list(p) for p in KEYWORDS], return_met=True)
    assert ids[ROW].tolist() == cids.tolist()
    assert met[ROW].tolist() == cmet.tolist()
    np.testing.assert_allclose(scores[ROW].cpu().numpy(), cscores, rtol=0, atol=1e-3)
    assert any(("kw", 2) in k for k in dec.graphs)
    sc = scores.cpu().numpy().astype(np.float64)
    assert np.isfinite(sc).all()
    np.testing.assert_allclose(rescore(model, tb, ids, L, model.engine().sh.V), sc, rtol=1e-3, atol=0)


# ------------------------------------------------------------------ 9. surfaces
def _ordered(met, scores):
    m, s = met.tolist(), scores.tolist()
    return all(m[i] > m[i + 1] or (m[i] == m[i + 1] and s[i] >= s[i + 1]) for i in range(len(m) - 1))


def test_keyword_surfaces():
    model, tb = build(CASE, "f32")                                   # (the mode in which the CPU search says every prompt holds both)
    n, length = tb["img_embs"].shape[0], 66
    kws = [list(p) for p in KEYWORDS]
    fresh, dec = BeamDecoder(model, n, NB, max_len=length), BeamDecoder(model, n, NB, max_len=length)
    # keywords=None is the call without the argument: ids, scores, graph keys
    i0, s0 = fresh.generate(tb, length, temperature=T, repitition_penalty=REP)
    i1, s1 = dec.generate(tb, length, temperature=T, repitition_penalty=REP, keywords=None)
    assert torch.equal(i0, i1) and torch.equal(s0, s1) and set(dec.graphs) == set(fresh.graphs) and dec.rules.kw is None
    keys = set(dec.graphs)
    ids, scores, met = dec.generate(tb, length, temperature=T, repitition_penalty=REP, keywords=kws, return_met=True)
    new = set(dec.graphs) - keys
    assert new and all(k[0] and ("kw", 2) in k for k in new)         # head steps only; the others replay the graphs they had
    ie, se = dec.generate(tb, length, temperature=T, repitition_penalty=REP, keywords=kws, use_graph=False)
    assert torch.equal(ie, ids) and torch.equal(se, scores)
    assert met.dtype == torch.int64 and tuple(met.shape) == (n, NB)
    for r in range(n):
        assert met[r].tolist() == [keywords_met(ids[r, k].tolist(), KEYWORDS) for k in range(NB)]
        assert _ordered(met[r], scores[r]), r
    assert int(met[:, 0].min()) == 2                                  # every prompt's first hypothesis holds both
    assert torch.isfinite(scores).all() and not torch.equal(ids, i0)
    i3, s3 = dec.generate(tb, length, temperature=T, repitition_penalty=REP)                  # and back
    assert torch.equal(i3, i0) and torch.equal(s3, s0) and dec.rules.kw is None
    # a whole given first line that holds a keyword: met from the start, and not written again
    line = [1, 30, KEYWORDS[0][0], KEYWORDS[0][1], 31] + [0] * (CAP - 4) + [2]
    ids, scores, met = dec.generate(tb, length, temperature=T, repitition_penalty=REP, keywords=kws, return_met=True, prefix=[line] * n)
    flat = ids.reshape(n * NB, -1).cpu().tolist()
    assert all(r[:SENT] == line for r in flat) and int(met.min()) >= 1
    assert all(keywords_met(r[SENT:], [KEYWORDS[0]]) == 0 for r in flat)
    assert any("prefix" in k and ("kw", 2) in k for k in dec.graphs)
    # with n-gram bans and line bounds: neither is broken (best effort: how many keywords fit is reported, not promised)
    ng = 3
    ids, scores, met = dec.generate(tb, length, temperature=T, repitition_penalty=REP, keywords=kws, return_met=True,
                                    no_repeat_ngram_size=ng, line_lengths=(3, 18))
    for r in ids.reshape(n * NB, -1).cpu().tolist():
        assert violations(r, ng) == [] and not repeated_ngrams(r, ng)
        for s in range(0, length + 1 - SENT, SENT):
            content = r[s + 1:s + SENT - 1]
            k = sum(1 for v in content if v != 0)
            assert 3 <= k <= 18 and all(v != 0 for v in content[:k]), (s, content)
    assert all(_ordered(met[r], scores[r]) for r in range(n))
    # (best effort in general; here the CPU search under the same constraints finds both keywords for prompt 0, over a run with no
    #  near-tie: tests/test_keywords_cpu.py::test_keywords_are_still_found_under_ngram_bans_and_line_bounds)
    assert int(met[0, 0]) >= 1 and int(met[:, 0].max()) >= 1
    assert met.tolist() == [[keywords_met(r, KEYWORDS) for r in p] for p in ids.cpu().tolist()]
    assert any(("kw", 2) in k and "lines" in k for k in dec.graphs)
    # the refused combinations
    for bad, match in ((dict(num_beam_groups=2, diversity_penalty=0.5), "both allocate"), (dict(return_logprobs=True), "no return_logprobs")):
        with pytest.raises(ValueError, match=match):
            dec.generate(tb, length, keywords=kws, **bad)


def test_generate_beams_with_keywords_returns_texts_that_contain_the_words():
    from mmtg_amd.generate import encode_keywords, generate_beams
    model, tb = build(CASE, "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

        def convert_tokens_to_ids(self, ch):
            return ord(ch) - 0x4e00 if 0 <= ord(ch) - 0x4e00 < 160 else 100

    words = ["".join(chr(0x4e00 + v) for v in p) for p in KEYWORDS]
    kws = encode_keywords(Tok(), words, vocab_cut=160)
    assert kws == [tuple(p) for p in KEYWORDS]
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    texts = generate_beams(model, rows, Tok(), num_beams=NB, length=66, keywords=kws)
    assert len(texts) == 3 and all(w in t for t in texts for w in words)
    plain = generate_beams(model, rows, Tok(), num_beams=NB, length=66)
    assert not any(w in t for t in plain for w in words)
    allb = generate_beams(model, rows, Tok(), num_beams=NB, length=66, keywords=[kws, kws[:1], kws], return_all=True, return_met=True,
                          max_batch=8)                              # one list per prompt, two prompts per chunk
    assert [b[0][0] for b in allb][::2] == texts[::2] and [len(b) for b in allb] == [NB] * 3
    assert all(b[-1] == sum(w in b[0] for w in words[:1 if r == 1 else 2]) for r, beams in enumerate(allb) for b in beams)
    assert allb[1][0][-1] == 1
