"""Diverse beam search on the MI355X (BeamDecoder with num_beam_groups / diversity_penalty): the grouped merge kernel against a host
restatement of the rule, one group against the plain merge, the decoder against the CPU search of tests/test_groups_cpu.py, and the
surfaces above it (return_groups, generate_beams(best_per_group=True))."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_lines  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case, start_row  # noqa: E402
from test_beam_gpu import build, rescore  # noqa: E402
from test_groups_cpu import FULL, G2, LAM, NB, NOT_CONTENT, REP, T, cpu_group_beam_search, group_select  # noqa: E402
from test_lines_cpu import CAP  # noqa: E402
from test_ngram_cpu import repeated_ngrams, violations  # noqa: E402
from test_rhyme_cpu import fixture_rhymes, followers_rhyme, rhyme_violations  # noqa: E402
from test_template_cpu import content_ids  # noqa: E402

DEV = "cuda"
NEG = np.float32(-np.inf)
P, TMAX, POS = 5, 48, 37
POOL = [0, 7, 11, 23, 42, 57, 100, 131]                     # candidate ids: PAD and [UNK] (exempt) among six content ids


# ------------------------------------------------------------------ 1. the kernel
def _tables(nb, n=3, seed=0):
    """Host inputs of one merge over n prompts: candidate tables over POOL (ids repeat across parents, so penalties fire) with
    -inf entries, one NaN and one dead parent, and random seq / keep / rows."""
    g = torch.Generator().manual_seed(100 * nb + seed)
    B = n * nb
    cv = -torch.rand(B, nb, generator=g) * 3
    cv = torch.sort(cv, dim=1, descending=True).values             # (ranks as the candidates kernel gives them: best first)
    cv[torch.rand(B, nb, generator=g) < 0.1] = float("-inf")
    cv[nb, 0] = float("nan")                                       # prompt 1, parent 0, rank 0
    ci = torch.tensor(POOL, dtype=torch.int32)[torch.randint(0, len(POOL), (B, nb), generator=g)]
    scores = -torch.rand(B, generator=g) * 2
    scores[2 * nb + nb - 1] = float("-inf")                        # prompt 2: its last parent is dead
    seq = torch.randint(3, 99, (B, TMAX), generator=g)
    keep = torch.randint(0, 2, (B, TMAX), generator=g, dtype=torch.int32)
    rows = torch.randint(0, B, (B, TMAX), generator=g, dtype=torch.int32)
    return cv, ci, scores, seq, keep, rows


def _restate(cv, ci, scores, seq, keep, rows, pos, nb, G, lam, held=()):
    """The rule of include/mmtg_hip.h on host copies (group_select of tests/test_groups_cpu.py is the selection)."""
    s = nb // G
    out = [t.clone() for t in (scores, seq, keep, rows)]
    osc, oseq, okeep, orows = out
    cvn, scn = cv.numpy(), scores.numpy()
    for b0 in range(0, seq.shape[0], nb):
        if b0 // nb in held:
            orows[b0:b0 + nb, pos + 1] = torch.arange(b0, b0 + nb, dtype=torch.int32)
            continue
        placed, r = [], 0
        for g in range(G):
            cands = []
            for p in range(g * s, (g + 1) * s):
                for k in range(nb):
                    base = np.float32(scn[b0 + p] + cvn[b0 + p, k])
                    cands.append((NEG if np.isnan(base) else base, p, k, int(ci[b0 + p, k])))
            for _, p, _, sc, v in group_select(cands, placed, s, lam)[0]:
                b, src = b0 + r, b0 + p
                oseq[b, :pos + 1], okeep[b, :pos + 1], orows[b, :pos + 1] = seq[src, :pos + 1], keep[src, :pos + 1], rows[src, :pos + 1]
                oseq[b, pos + 1], orows[b, pos + 1], osc[b] = v, b, float(sc)
                placed.append((v, sc))
                r += 1
    return out


def _run(entry, cv, ci, scores, seq, keep, rows, pos, nb, *tail):
    d = [None if t is None else t.to(DEV) for t in (cv, ci, scores, seq, keep, rows)]
    posd = torch.tensor([pos, -7], dtype=torch.int32, device=DEV)
    entry(d[0], d[1], d[2], d[3], d[4], d[5], posd[0:1], P, SENT, nb, seq.shape[0] // nb, *tail, pos_next=posd[1:2])
    torch.cuda.synchronize()
    assert int(posd[1]) == pos + 1
    return [t.cpu() for t in d[2:]]


def _same(got, want):
    return all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("nb,G", [(4, 2), (4, 4), (6, 3), (16, 4), (16, 1)])
def test_grouped_merge_is_the_host_restatement(nb, G):
    cv, ci, scores, seq, keep, rows = _tables(nb)
    fired = 0
    for lam in (0.5, 1e4, 0.0):
        want = _restate(cv, ci, scores, seq, keep, rows, POS, nb, G, lam)
        got = _run(hip.decode_beam_merge_groups, cv, ci, scores, seq, keep, rows, POS, nb, G, lam)
        assert _same(got, want), (nb, G, lam)
        fired += want[1][:, POS + 1].tolist() != _restate(cv, ci, scores, seq, keep, rows, POS, nb, G, 0.0)[1][:, POS + 1].tolist()
        # the *_fixed entry: prompt 1 held, and left as the plain *_fixed merge leaves it; the others as above
        fe = torch.full((3 * nb,), P + 1, dtype=torch.int32)
        fe[nb:2 * nb] = POS + 2
        got = _run(hip.decode_beam_merge_groups_fixed, cv, ci, scores, seq, keep, rows, POS, nb, fe.to(DEV), G, lam)
        assert _same(got, _restate(cv, ci, scores, seq, keep, rows, POS, nb, G, lam, held=(1,))), (nb, G, lam)
        plain = _run(hip.decode_beam_merge_fixed, cv, ci, scores, seq, keep, rows, POS, nb, fe.to(DEV))
        assert _same([t[nb:2 * nb] for t in got], [t[nb:2 * nb] for t in plain])
    assert G == 1 or fired >= 1                                     # the penalty changed what some group took
    # PAD and [UNK] are never penalised: with every candidate one of them, the groups choose as at penalty 0
    ex = ci.clone()
    ex[ex % 2 == 1] = 0
    ex[(ex != 0) & (ex != 100)] = 100
    assert set(ex.unique().tolist()) <= set(NOT_CONTENT)
    got = _run(hip.decode_beam_merge_groups, cv, ex, scores, seq, keep, rows, POS, nb, G, 1e4)
    assert _same(got, _restate(cv, ex, scores, seq, keep, rows, POS, nb, G, 0.0))


# ------------------------------------------------------------------ 2. one group is the plain merge
@pytest.mark.parametrize("nb", [1, 4, 16])
def test_one_group_is_the_plain_merge_bit_for_bit(nb):
    cv, ci, scores, seq, keep, rows = _tables(nb, seed=1)
    for pos in (POS, P + 20, P + 21):                               # a selection, a forced [#EOS#], a forced [#START#]
        want = _run(hip.decode_beam_merge, cv, ci, scores, seq, keep, rows, pos, nb)
        for lam in (0.0, 0.7, 1e4):
            assert _same(_run(hip.decode_beam_merge_groups, cv, ci, scores, seq, keep, rows, pos, nb, 1, lam), want), (pos, lam)
    want = _run(hip.decode_beam_merge, None, None, scores, seq, keep, rows, POS, nb)          # a step without the head
    assert _same(_run(hip.decode_beam_merge_groups, None, None, scores, seq, keep, rows, POS, nb, nb, 0.5), want)


# ------------------------------------------------------------------ 3. the decoder follows the CPU search
@functools.lru_cache(maxsize=None)
def _cpu_run(case, row, length):
    """The CPU search of one prompt (computed once, shared by the modes)."""
    fx, sh, w, table, batch = _case(case)
    return cpu_group_beam_search(w, sh, table, start_row(batch, row), length, NB, G2, LAM, T, REP)


@functools.lru_cache(maxsize=None)
def _case(case):
    return setup_case(case)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", ["tiny_s5", "tiny_lstm2_rnn2"])
def test_four_beams_in_two_groups_follow_the_cpu_search(case, mode):
    """Every prompt is compared over the generated positions before its first CPU group selection whose s-th / (s+1)-th gap is
    below 1e-4: ids, order and groups equal, scores within 1e-3 (the bounds of test_four_beams_follow_the_cpu_beam_search)."""
    model, tb = build(case, mode)
    n = tb["img_embs"].shape[0]
    lens = [comparable_length(_cpu_run(case, row, FULL)[2], FULL) for row in range(n)]
    assert max(lens) >= 40, lens
    dec = BeamDecoder(model, n, NB, max_len=FULL)
    runs = {}
    for row, L in enumerate(lens):
        if L < 1:
            continue
        if L not in runs:
            runs[L] = [t.cpu() for t in dec.generate(tb, L, temperature=T, repitition_penalty=REP, num_beam_groups=G2,
                                                     diversity_penalty=LAM, return_groups=True)]
        ids, scores, groups = runs[L]
        cids, cscores, _, cgroups = _cpu_run(case, row, L)
        assert ids[row].tolist() == cids.tolist(), (row, L)
        assert groups[row].tolist() == cgroups.tolist(), (row, L)
        np.testing.assert_allclose(scores[row].numpy(), cscores, rtol=0, atol=1e-3)
    assert any(("groups", G2, LAM) in k for k in dec.graphs)


# ------------------------------------------------------------------ 4. the first free column
@pytest.mark.parametrize("nb,G", [(4, 4), (6, 3)])
def test_a_huge_penalty_gives_every_beam_its_own_first_id(nb, G):
    """One generated column, so the beams are read as the first selection left them (later selections of a group of two may
    keep two children of one parent, which share its first id): every group takes ids no earlier group took -- nb distinct ids
    are always on offer, the containment guarantee."""
    model, tb = build("tiny_s5", "f32")
    n = tb["img_embs"].shape[0]
    ids, scores = BeamDecoder(model, n, nb, max_len=8).generate(tb, 1, temperature=T, repitition_penalty=REP, num_beam_groups=G,
                                                                diversity_penalty=1e4)
    assert tuple(ids.shape) == (n, nb, 2)
    first = ids[:, :, 1].cpu()
    for r in range(n):
        assert len(set(first[r].tolist())) == nb, (r, first[r].tolist())
    assert torch.isfinite(scores).all() and (scores > -1e3).all()         # the penalty is not in the scores


# ------------------------------------------------------------------ 5. scores are the unpenalised sums
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_grouped_scores_rescore_through_the_greedy_decoder(mode):
    nb, length = 4, 120
    model, tb = build("tiny_s5", mode)
    n = tb["img_embs"].shape[0]
    ids, scores, groups = BeamDecoder(model, n, nb, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP,
                                                                             num_beam_groups=2, diversity_penalty=1.0, return_groups=True)
    sc = scores.cpu().numpy().astype(np.float64)
    assert np.isfinite(sc).all() and (np.diff(sc, axis=1) <= 0).all()
    assert all(sorted(r) == [0, 0, 1, 1] for r in groups.tolist())
    got = rescore(model, tb, ids, length, model.engine().sh.V)
    np.testing.assert_allclose(got, sc, rtol=1e-3, atol=0)


# ------------------------------------------------------------------ 6. one group changes nothing
def test_one_group_is_exactly_the_call_without_the_argument():
    model, tb = build("tiny_s5", "bf16")
    n = tb["img_embs"].shape[0]
    fresh, dec = BeamDecoder(model, n, 4, max_len=66), BeamDecoder(model, n, 4, max_len=66)
    i0, s0 = fresh.generate(tb, 66, temperature=T, repitition_penalty=REP)
    i1, s1, g1 = dec.generate(tb, 66, temperature=T, repitition_penalty=REP, num_beam_groups=1, diversity_penalty=0.0, return_groups=True)
    assert torch.equal(i0, i1) and torch.equal(s0, s1) and set(dec.graphs) == set(fresh.graphs) and int(g1.abs().max()) == 0
    assert g1.dtype == torch.int64 and tuple(g1.shape) == (n, 4)
    keys = set(dec.graphs)
    i2, s2 = dec.generate(tb, 66, temperature=T, repitition_penalty=REP, num_beam_groups=2, diversity_penalty=0.5)
    new = set(dec.graphs) - keys
    assert new and all(k[0] and ("groups", 2, 0.5) in k for k in new)      # head steps only; the others replay the graphs they had
    assert not torch.equal(i2, i0)
    i3, s3 = dec.generate(tb, 66, temperature=T, repitition_penalty=REP)                      # and back
    assert torch.equal(i3, i0) and torch.equal(s3, s0) and dec.rules.groups == 1


# ------------------------------------------------------------------ 7. with the constraints
def test_groups_compose_with_a_prefix_ngram_bans_line_bounds_and_a_rhyme_scheme():
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "f32")
    cid = content_ids(fx)
    classes, bounds = fixture_rhymes(fx)
    line = [1, cid[20], cid[21], cid[5]] + [0] * (CAP - 3) + [2]               # a whole first line of the caller's (three tokens)
    pre = [line, line, line]
    length, n, nb, G = 4 * SENT, 3, 4, 2
    kw = dict(line_lengths=bounds, rhyme_scheme="AABB", rhyme_classes=classes, no_repeat_ngram_size=n, prefix=pre, num_beam_groups=G,
              diversity_penalty=1.0)
    tabs = check_lines(bounds, None, 3, length, SENT, 160, prefix=pre, rhyme_scheme="AABB", rhyme_classes=classes)
    dec = BeamDecoder(model, 3, nb, max_len=length)
    ids, scores, groups = dec.generate(tb, length, temperature=T, repitition_penalty=REP, return_groups=True, **kw)
    ids2, scores2, groups2 = dec.generate(tb, length, temperature=T, repitition_penalty=REP, return_groups=True, **kw)
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2) and torch.equal(groups, groups2)
    ie, se = dec.generate(tb, length, temperature=T, repitition_penalty=REP, use_graph=False, **kw)
    assert torch.equal(ie, ids) and torch.equal(se, scores)
    flat = ids.reshape(3 * nb, -1).cpu()
    rhymed = 0
    for r in range(3 * nb):
        row = flat[r].tolist()
        assert row[:len(line)] == line, r                                      # the prefix columns
        assert violations(row, n, start=len(line)) == [] and not repeated_ngrams(row, n), r
        assert rhyme_violations(row, tabs, r // nb, start=len(line), n=n) == [], r            # the bounds and the scheme
        pairs = followers_rhyme(row, tabs, r // nb)
        assert all(ok for _, _, ok in pairs), (r, pairs)
        rhymed += len(pairs)
    assert rhymed >= 3 * nb
    assert all(sorted(g) == [0, 0, 1, 1] for g in groups.tolist())
    assert torch.isfinite(scores).all() and (scores[:, :-1] >= scores[:, 1:]).all()
    assert any("prefix" in k and ("groups", G, 1.0) in k for k in dec.graphs)  # the held, grouped merge ran


# ------------------------------------------------------------------ 8. the text surface
def test_generate_beams_best_per_group():
    from mmtg_amd.generate import generate_beams
    model, tb = build("tiny_s5", "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    for nb, G in ((4, 2), (4, 4)):
        kw = dict(num_beams=nb, length=44, num_beam_groups=G, diversity_penalty=1.0)
        allb = generate_beams(model, rows, Tok(), return_all=True, return_ids=True, **kw)
        best = generate_beams(model, rows, Tok(), best_per_group=True, **kw)
        with_ids = generate_beams(model, rows, Tok(), best_per_group=True, return_ids=True, **kw)
        ids, scores, groups = BeamDecoder(model, 3, nb, max_len=44).generate(tb, 44, temperature=1.1, repitition_penalty=1.5, num_beam_groups=G,
                                                                            diversity_penalty=1.0, return_groups=True)
        assert len(best) == 3
        for r in range(3):
            assert [b[2] for b in allb[r]] == ids[r].tolist() and [b[1] for b in allb[r]] == [float(v) for v in scores[r]]
            where = [groups[r].tolist().index(g) for g in range(G)]            # best first: a group's first place is its best
            assert best[r] == [allb[r][i][:2] for i in where] and len(best[r]) == G
            assert with_ids[r] == [allb[r][i] for i in where]
    assert generate_beams(model, rows, Tok(), num_beams=4, length=44) == [b[0][0] for b in generate_beams(model, rows, Tok(), num_beams=4, length=44, return_all=True)]
