"""Diverse beam search (BeamDecoder with num_beam_groups / diversity_penalty): the rule restated on the CPU, the containment
argument the merge rests on, and the host side of the two new ABI entries.

`cpu_group_beam_search` is tests/test_beam_cpu.py's search with the beams in G groups served in order, a later group lowered by
lambda per earlier group's live slot that took the same content id at the step (include/mmtg_hip.h states the rule).  At G = 1 it
must be `cpu_beam_search` itself.  tests/test_groups_gpu.py holds the decoder to it."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, StepRules, check_groups, select_forms
from oracle import mmtg_oracle as O
from test_beam_cpu import NEG, SENT, _fork, comparable_length, cpu_beam_search, setup_case, start_row
from test_ngram_cpu import _Eng, _Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, REP = 1.1, 1.5
NOT_CONTENT = (0, 1, 2, 100, 102)
# the settings tests/test_groups_gpu.py follows the CPU search at: four beams in two groups; the penalty is the member of
# {0.5, 1.0, 2.0} at which each fixture keeps a comparable run of 40 columns or more (the last test below)
NB, G2, LAM, FULL = 4, 2, 1.0, 120


def group_select(cands, placed, s, lam):
    """One group's selection.  cands: (base, parent, rank, id) of the group's parents; placed: (id, stored score) of the slots
    earlier groups filled at this step.  Returns (the s kept candidates in order, the gap between the s-th and (s+1)-th sel)."""
    lam = np.float32(lam)
    keyed = []
    for base, p, k, v in cands:
        n = sum(1 for t, sc in placed if t == v and sc > NEG) if v not in NOT_CONTENT else 0
        sel = np.float32(base) - lam * np.float32(n) if n else np.float32(base)
        keyed.append((sel, p, k, np.float32(base), v))
    keyed.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
    gap = float(keyed[s - 1][0]) - float(keyed[s][0]) if len(keyed) > s else float("inf")
    return keyed[:s], gap


def cpu_group_beam_search(w, sh, table, start, length, nb, G, lam, temperature, repetition_penalty):
    """cpu_beam_search with `nb` beams in `G` groups and the penalty `lam`.  Returns (ids [nb, 1 + length], scores [nb] fp32, gaps,
    groups [nb]): the hypotheses best first by score (stable over the final rows, as BeamDecoder.generate orders them), gaps[c] =
    (lyric column appended, the gap between the s-th and (s+1)-th sel of one group's selection) for every selection and group in
    turn, groups[i] = the group of the hypothesis at place i."""
    assert nb % G == 0
    s = nb // G
    base = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in start.items() if k not in ("targets", "rating")}
    base["topic_ids"] = base["topic_ids"].long()
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    cf0 = O.CachedForward(w, sh, table)
    beams = [(cf0 if r == 0 else _fork(cf0), [1], np.float32(0.0) if r % s == 0 else NEG) for r in range(nb)]
    gaps = []
    for i in range(length):
        if i > 0 and (i + 2) % SENT in (0, 1):
            tok = 2 if (i + 2) % SENT == 0 else 1
            beams = [(cf, ids + [tok], sc) for cf, ids, sc in beams]
            continue
        cands = []                                                 # per parent: (base, parent, rank, token)
        for p, (cf, ids, sc) in enumerate(beams):
            if sc == NEG:
                cands.append([(NEG, p, k, 0) for k in range(nb)])
                continue
            inputs = dict(base, targets=torch.tensor([ids], dtype=torch.long))
            logits = cf(inputs)[0, -1, :]
            if ids[-1] == 0:
                cands.append([(sc, p, 0, 0)] + [(NEG, p, k, 0) for k in range(1, nb)])
                continue
            x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V]
            lp = torch.log_softmax(x, -1)
            order = torch.sort(x, descending=True, stable=True).indices[:nb]
            cands.append([(np.float32(sc + np.float32(lp[v].item())), p, k, int(v)) for k, v in enumerate(order.tolist())])
        new, placed = [], []
        for g in range(G):
            kept, gap = group_select([c for p in range(g * s, (g + 1) * s) for c in cands[p]], placed, s, lam)
            if nb > 1:
                gaps.append((len(beams[0][1]), gap))
            for _, p, _, sc, tok in kept:
                new.append((_fork(beams[p][0]), beams[p][1] + [tok], sc))
                placed.append((tok, sc))
        beams = new
    scores = np.array([sc for _, _, sc in beams], np.float32)
    order = sorted(range(nb), key=lambda r: -float(scores[r]))      # (sorted is stable: ties keep the lower final row first)
    return np.array([beams[r][1] for r in order]), scores[order], gaps, np.array([r // s for r in order])


# ------------------------------------------------------------------ 1. the reference search
@pytest.mark.parametrize("case", ["tiny_s5", "tiny_lstm2_rnn2"])
def test_one_group_is_the_plain_cpu_beam_search(case):
    fx, sh, w, table, batch = setup_case(case)
    for row, length in ((0, 66), (2, 30)):
        ids, scores, gaps = cpu_beam_search(w, sh, table, start_row(batch, row), length, 4, T, REP)
        gids, gscores, ggaps, groups = cpu_group_beam_search(w, sh, table, start_row(batch, row), length, 4, 1, 0.0, T, REP)
        assert gids.tolist() == ids.tolist() and gscores.tobytes() == scores.tobytes() and ggaps == gaps
        assert groups.tolist() == [0, 0, 0, 0]


def test_groups_search_on_their_own_and_the_penalty_parts_them():
    """Four beams in four groups: at penalty 0 every group runs the greedy search of its own start beam, so all four hypotheses are
    the one-beam search's; a huge penalty gives four different ids at the first free column, and the scores are still the
    unpenalised sums (finite, and group 0 -- never penalised -- is still the greedy hypothesis)."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    start, length = start_row(batch, 0), 30
    one, sc1, _ = cpu_beam_search(w, sh, table, start, length, 1, T, REP)
    ids, scores, _, groups = cpu_group_beam_search(w, sh, table, start, length, 4, 4, 0.0, T, REP)
    assert all(r == one[0].tolist() for r in ids.tolist()) and (scores == sc1[0]).all() and groups.tolist() == [0, 1, 2, 3]
    ids, scores, gaps, groups = cpu_group_beam_search(w, sh, table, start, length, 4, 4, 1e4, T, REP)
    assert len(set(ids[:, 1].tolist())) == 4 and sorted(groups.tolist()) == [0, 1, 2, 3]
    assert np.isfinite(scores).all() and (scores > -1e3).all() and (np.diff(scores) <= 0).all()
    assert ids[groups.tolist().index(0)].tolist() == one[0].tolist()
    assert len(gaps) == 4 * sum(1 for i in range(length) if not (i > 0 and (i + 2) % SENT in (0, 1)))


# ------------------------------------------------------------------ 2. the candidates' top nb per parent is enough
def _full_or_cut(rows, scores, parents, placed, s, lam, limit):
    """group_select over the parents' whole rows (limit None) or over their best `limit` ids; ranks are the unpenalised ones."""
    cands = []
    for p in parents:
        order = np.argsort(-rows[p], kind="stable")
        for k, v in enumerate(order[:limit].tolist() if limit else order.tolist()):
            cands.append((np.float32(scores[p] + rows[p, v]), p, k, v))
    kept, _ = group_select(cands, placed, s, lam)
    return [(p, v, sc.tobytes()) for _, p, _, sc, v in kept]


@pytest.mark.parametrize("nb", [4, 6, 16])
def test_selecting_from_each_parents_top_nb_is_selecting_from_the_whole_penalised_rows(nb):
    """Seeded fp32 log-probability rows without ties, V = 200 (the five exempt ids among them).  The parents' rows are one shared
    row plus small noise, so all parents agree on the top ids and what earlier groups placed sits at the top of every later row;
    the earlier groups' slots are once what the groups themselves selected and once drawn from the group's own top ids (dead slots
    among them).  Parents, ids and scores agree exactly for every group of every divisor G of nb."""
    V = 200
    rng = np.random.RandomState(nb)
    hits = 0
    for G in [g for g in range(1, nb + 1) if nb % g == 0]:
        s = nb // G
        for lam in (0.5, 3.0, 1e4):
            shared = rng.randn(V).astype(np.float32) * 3
            rows = (shared[None, :] + rng.randn(nb, V).astype(np.float32) * 0.2).astype(np.float32)
            rows -= np.log(np.exp(rows.astype(np.float64)).sum(1, keepdims=True)).astype(np.float32)
            scores = (-rng.rand(nb) * 2).astype(np.float32)
            assert all(len(set(r.tolist())) == V for r in rows)
            placed = []
            for g in range(G):
                parents = list(range(g * s, (g + 1) * s))
                full = _full_or_cut(rows, scores, parents, placed, s, lam, None)
                assert _full_or_cut(rows, scores, parents, placed, s, lam, nb) == full, (G, lam, g)
                top = {int(v) for p in parents for v in np.argsort(-rows[p], kind="stable")[:s + 1]}
                hits += sum(1 for t, _ in placed if t in top)
                # drawn slots: g * s ids from the tops of this group's own rows, one of them dead
                pool = sorted(top)
                drawn = [(pool[i % len(pool)], NEG if i == 1 else np.float32(-1.0)) for i in rng.permutation(g * s)]
                full_d = _full_or_cut(rows, scores, parents, drawn, s, lam, None)
                assert _full_or_cut(rows, scores, parents, drawn, s, lam, nb) == full_d, (G, lam, g, "drawn")
                placed += [(v, np.frombuffer(sc, np.float32)[0]) for _, v, sc in full]
            if G == nb and lam == 1e4:                                # one beam per group: nb distinct ids were on offer, and taken
                content = [t for t, _ in placed if t not in NOT_CONTENT]
                assert len(set(content)) == len(content)
    assert nb == 1 or hits > 0                                        # the penalties did hit the top of the rows


# ------------------------------------------------------------------ 3. entry points and validation
def test_group_entry_points_are_declared_exported_bound_and_reject_bad_arguments_without_a_gpu():
    L = hip.lib()
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    for name in ("mmtg_decode_beam_merge_groups", "mmtg_decode_beam_merge_groups_fixed"):
        assert "MMTG_API int %s(" % name in header
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
        assert len(hip._SIGS[name][0]) == len(hip._SIGS[name.replace("_groups", "")][0]) + 2
    assert callable(hip.decode_beam_merge_groups) and callable(hip.decode_beam_merge_groups_fixed)
    assert L.mmtg_abi_version() == hip.ABI_VERSION == 12
    p = [0x7000000000 + (i << 24) for i in range(10)]

    def plain(nb, groups, lam):
        return L.mmtg_decode_beam_merge_groups(p[0], p[1], p[2], p[3], 64, p[4], 64, p[5], 64, p[6], 5, SENT, nb, 2, p[7], groups, lam, None)

    def fixed(nb, groups, lam, fe=p[8]):
        return L.mmtg_decode_beam_merge_groups_fixed(p[0], p[1], p[2], p[3], 64, p[4], 64, p[5], 64, p[6], 5, SENT, nb, 2, p[7], fe, groups,
                                                     lam, None)
    for entry, what in ((plain, b"decode_beam_merge_groups"), (fixed, b"decode_beam_merge_groups_fixed")):
        for nb in (0, 17):
            assert entry(nb, 1, 0.0) == -1 and what + b": %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
        for nb, groups in ((4, 0), (4, -1), (4, 3), (4, 8), (6, 4), (16, 5)):
            assert entry(nb, groups, 0.5) == -1
            assert what + b": %d groups do not divide %d beams" % (groups, nb) in L.mmtg_last_error()
        for lam in (-0.5, float("nan"), float("inf"), -float("inf")):
            assert entry(4, 2, lam) == -1 and what + b": diversity penalty must be finite and >= 0" in L.mmtg_last_error()
    assert fixed(4, 2, 0.5, fe=None) == -1 and b"decode_beam_merge_groups_fixed: null fixed_end" in L.mmtg_last_error()


def test_check_groups():
    assert check_groups(4) == (1, 0.0) and check_groups(4, 2, 0.5) == (2, 0.5) and check_groups(16, 16, 0) == (16, 0.0)
    assert check_groups(6, np.int64(3), np.float32(2.0)) == (3, 2.0) and check_groups(4, 2) == (2, 0.0)
    for nb, G in ((4, 3), (4, 0), (4, -2), (4, 8), (6, 4), (4, 2.0), (4, True), (4, None)):
        with pytest.raises(ValueError, match="num_beam_groups"):
            check_groups(nb, G, 0.0)
    for lam in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="diversity_penalty"):
            check_groups(4, 2, lam)
    with pytest.raises(ValueError, match="diversity_penalty .* needs num_beam_groups > 1"):
        check_groups(4, 1, 0.5)


def test_decoder_and_generate_beams_reject_bad_groups_before_any_device_work():
    from mmtg_amd.generate import generate_beams
    rows = {"topic_ids": np.zeros((1, 5), np.int64)}
    bad = ((dict(num_beam_groups=3), "num_beam_groups"), (dict(num_beam_groups=0), "num_beam_groups"),
           (dict(num_beam_groups=-1), "num_beam_groups"), (dict(num_beam_groups=8), "num_beam_groups"),
           (dict(num_beam_groups=2, diversity_penalty=-0.5), "diversity_penalty"),
           (dict(num_beam_groups=2, diversity_penalty=float("nan")), "diversity_penalty"),
           (dict(num_beam_groups=2, diversity_penalty=float("inf")), "diversity_penalty"),
           (dict(num_beam_groups=1, diversity_penalty=0.5), "needs num_beam_groups > 1"), (dict(diversity_penalty=1.0), "needs num_beam_groups > 1"))
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            generate_beams(_Model(), rows, None, num_beams=4, **kw)
        dec = BeamDecoder.__new__(BeamDecoder)
        dec.eng = _Eng()
        dec.B, dec.max_len, dec.n_prompts, dec.nb = 4, 220, 1, 4
        with pytest.raises(ValueError, match=match):
            dec.begin({"img_embs": torch.zeros(1, 4)}, 220, **kw)
        with pytest.raises(ValueError, match=match):
            dec.generate({"img_embs": torch.zeros(1, 4)}, 220, **kw)
        for good in (dict(num_beam_groups=2, diversity_penalty=0.5), dict(num_beam_groups=2, diversity_penalty=0.5, return_groups=True)):
            with pytest.raises(ValueError, match="no return_logprobs"):                  # still refused, groups or not
                dec.generate({"img_embs": torch.zeros(1, 4)}, 220, return_logprobs=True, **good)
        with pytest.raises(ValueError, match="no return_logprobs"):
            dec.begin({"img_embs": torch.zeros(1, 4)}, 220, return_logprobs=True, num_beam_groups=2, diversity_penalty=0.5)
    with pytest.raises(ValueError, match="best_per_group"):
        generate_beams(_Model(), rows, None, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, best_per_group=True, return_all=True)
    with pytest.raises(ValueError, match="best_per_group"):
        generate_beams(_Model(), rows, None, num_beams=4, best_per_group=True, return_all=True)
    g = GreedyDecoder.__new__(GreedyDecoder)                       # the greedy decoder has no groups to take
    with pytest.raises(TypeError, match="num_beam_groups"):
        g.generate({"img_embs": torch.zeros(1, 4)}, 220, num_beam_groups=2)


# ------------------------------------------------------------------ 4. which merge a step ends in
def test_select_forms_names_the_grouped_merge_on_head_steps_only(monkeypatch):
    from types import SimpleNamespace as NS
    for with_head in (True, False):
        for prefix in (False, True):
            for ngram in (0, 3):
                for lines in (False, True):
                    for templates in (False, True):
                        for rhymes in (False, True):
                            was = select_forms(with_head, prefix, ngram, lines, templates=templates, rhymes=rhymes)
                            assert select_forms(with_head, prefix, ngram, lines, templates=templates, rhymes=rhymes, groups=False) == was
                            held = "_fixed" if prefix else ""
                            got = select_forms(with_head, prefix, ngram, lines, templates=templates, rhymes=rhymes, groups=True)
                            assert got == ((was[0], "_groups" + held) if with_head else was)
    calls = []

    class Lib:
        def __getattr__(self, name):
            def entry(*a):
                assert len(a) == len(hip._SIGS[name][0]), name
                calls.append((name, a))
                return 0
            return entry
    monkeypatch.setattr(hip, "lib", lambda: Lib())
    monkeypatch.setattr(hip, "_stream", lambda: 0)
    B, nb, V = 8, 4, 160
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                        # noqa: E731
    for with_head in (True, False):
        for prefix in (False, True):
            for ngram in (0, 3):
                for G, lam in ((1, 0.0), (2, 0.5), (4, 0.0)):
                    fe = i32(B)
                    dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, nb=nb, n_prompts=B // nb,
                             rules=StepRules(prefix=prefix, ngram=ngram, groups=G, diversity_penalty=lam), copy_step=False, fixed_end=fe,
                             logits=torch.zeros(B, V),
                             seq=torch.zeros(B, 64, dtype=torch.long), pos=i32(1), pos_next=i32(1), keep=i32(B, 64), rows=i32(B, 64),
                             scores=torch.zeros(B), cand_val=torch.zeros(B, nb), cand_id=i32(B, nb), params=(1.1, 1.5, 1, 0.0))
                    held = "_fixed" if prefix else ""
                    base = (with_head, 0, dec.params) + (("prefix",) if prefix else ()) + (("ngram", 3) if ngram else ())
                    key = GreedyDecoder._graph_key(dec, with_head, 0)
                    assert key == base + ((("groups", G, float(lam)),) if with_head and G > 1 else ())
                    del calls[:]
                    BeamDecoder._select(dec, with_head)
                    cand = "_ngram" if ngram else held
                    merge = ("_groups" if with_head and G > 1 else "") + held
                    assert [c[0] for c in calls] == (["mmtg_decode_beam_candidates" + cand] if with_head else []) + ["mmtg_decode_beam_merge" + merge]
                    a = calls[-1][1]
                    if with_head and G > 1:
                        assert a[-3:] == (G, lam, 0) and (not prefix or a[-4] == fe.data_ptr())
                    else:                                              # the entries and the arguments a search without groups has
                        assert a[-2:] == ((fe.data_ptr(), 0) if prefix else (dec.pos_next.data_ptr(), 0))


# ------------------------------------------------------------------ 5. the fixtures give the GPU comparison enough to compare
@pytest.mark.parametrize("case", ["tiny_s5", "tiny_lstm2_rnn2"])
def test_grouped_cpu_search_rules_and_comparable_length(case):
    """Four beams in two groups at the penalty tests/test_groups_gpu.py uses: the forced cadence on every beam, two hypotheses per
    group, finite scores best first -- and some prompt of each fixture keeps 40 generated columns or more before the first group
    selection whose s-th / (s+1)-th gap is below 1e-4 (the condition of the GPU comparison, from the CPU reference alone)."""
    fx, sh, w, table, batch = setup_case(case)
    lens = []
    for row in range(batch["topic_ids"].shape[0]):
        ids, scores, gaps, groups = cpu_group_beam_search(w, sh, table, start_row(batch, row), FULL, NB, G2, LAM, T, REP)
        assert ids.shape == (NB, 1 + FULL) and (ids[:, 0] == 1).all()
        assert np.isfinite(scores).all() and (np.diff(scores) <= 0).all()
        assert sorted(groups.tolist()) == [0, 0, 1, 1]
        for g in range(G2):                                        # inside a group no duplicate hypotheses
            assert len({tuple(r) for r in ids[groups == g].tolist()}) == NB // G2
        for j in range(2, 1 + FULL):
            if (j + 1) % SENT == 0:
                assert (ids[:, j] == 2).all()
            elif (j + 1) % SENT == 1:
                assert (ids[:, j] == 1).all()
        lens.append(comparable_length(gaps, FULL))
    print(case, "comparable runs", lens)
    assert max(lens) >= 40, lens
