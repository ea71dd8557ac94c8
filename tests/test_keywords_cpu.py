"""Keyword-constrained beam search (BeamDecoder with keywords=): the host side of the three new ABI entries, the checks and packing
of the keywords, the bank and the selection rule restated on the host, and the CPU search that pins the decoder.

`cpu_keyword_beam_search` is tests/test_beam_cpu.py's search with the rule of include/mmtg_hip.h: every parent offers its top nb
and one slot per unmet keyword, every candidate carries bank(h + [id]), and the nb places go to the best of every bank, highest
bank first.  Without keywords it must be `cpu_beam_search` itself.  tests/test_keywords_gpu.py holds the decoder to it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.constraints import (KeywordTables, check_keywords, keyword_bank, keyword_met_mask, keyword_select, keywords_met)
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, StepRules, select_forms
from mmtg_amd.generate import encode_keywords, generate_beams, generate_samples
from oracle import mmtg_oracle as O
from test_beam_cpu import NEG, SENT, _fork, comparable_length, cpu_beam_search, setup_case, start_row
from test_ngram_cpu import _Eng, _Model, banned_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, REP = 1.1, 1.5
NOT_CONTENT = (0, 1, 2, 100, 102)
# what tests/test_keywords_gpu.py follows the CPU search at: fixture, prompt, four beams, two keywords (one of them two ids long)
# that the plain search of this prompt leaves out of all four hypotheses (asserted below), and the length of the run
CASE, ROW, NB, FULL = "tiny_s5", 1, 4, 66
KEYWORDS = ((144, 47), (148,))


def keyword_candidates(x, hist, sc, nb, phrases, V):
    """One parent's W = nb + K candidates (base, bank, token) at a free column: x the processed logits [V], hist the parent's lyric
    ids so far, sc its score."""
    lp = torch.log_softmax(x, -1)
    order = torch.sort(x, descending=True, stable=True).indices[:nb].tolist()
    out = []
    for v in order:
        if float(x[v]) == float("-inf"):
            out.append((NEG, 0, 0))
        else:
            out.append((np.float32(sc + np.float32(lp[v].item())), keyword_bank(hist + [v], phrases), int(v)))
    met = keyword_met_mask(hist, phrases)
    offered = []
    for p, m in zip(phrases, met):
        t = None
        if not m:
            prog = max([k for k in range(1, len(p)) if k <= len(hist) and tuple(hist[len(hist) - k:]) == tuple(p[:k])] + [0])
            t = p[prog]
        if t is None or t >= V or float(x[t]) == float("-inf") or t in order or t in offered:
            out.append((NEG, 0, 0))
        else:
            out.append((np.float32(sc + np.float32(lp[t].item())), keyword_bank(hist + [t], phrases), int(t)))
        offered.append(t)
    return out


def bank_gaps(cands, nb):
    """The smallest gap between two live candidates of one bank that are adjacent in the bank's order, one of them ranked below nb
    in its bank (inf if there is no such pair): closer than rounding, two fp32 searches may order them differently."""
    gap = float("inf")
    live = [(np.float32(b), bank) for b, bank, _ in cands if not np.isnan(b) and b > NEG]
    for bank in {k for _, k in live}:
        own = sorted((float(b) for b, k in live if k == bank), reverse=True)
        for r in range(min(nb, len(own) - 1)):
            gap = min(gap, own[r] - own[r + 1])
    return gap


def cpu_keyword_beam_search(w, sh, table, start, length, nb, phrases, temperature, repetition_penalty, ngram=0, bounds=None):
    """cpu_beam_search under keywords; ngram: no_repeat_ngram_size, bounds: line_lengths=(lo, hi) for every line (bans win over
    keywords: a banned id's processed logit is -inf before the slots are filled; a full line offers PAD alone).  Returns (ids [nb, 1 + length], scores [nb] fp32, gaps, met [nb]): the hypotheses ordered by
    (keywords met descending, score descending, stable over the final rows), gaps[c] = (lyric column appended, bank_gaps of that
    selection), met[i] = the number of keywords hypothesis i holds."""
    phrases = [tuple(p) for p in phrases]
    base = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in start.items() if k not in ("targets", "rating")}
    base["topic_ids"] = base["topic_ids"].long()
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    W = nb + len(phrases)
    cf0 = O.CachedForward(w, sh, table)
    beams = [(cf0, [1], np.float32(0.0))] + [(_fork(cf0), [1], NEG) for _ in range(nb - 1)]
    gaps = []
    for i in range(length):
        if i > 0 and (i + 2) % SENT in (0, 1):
            tok = 2 if (i + 2) % SENT == 0 else 1
            beams = [(cf, ids + [tok], s) for cf, ids, s in beams]
            continue
        cands = []
        for p, (cf, ids, s) in enumerate(beams):
            if s == NEG:
                cands += [(NEG, 0, 0)] * W
                continue
            logits = cf(dict(base, targets=torch.tensor([ids], dtype=torch.long)))[0, -1, :]
            if ids[-1] == 0:                                       # sticky PAD: one candidate, the score unchanged
                cands += [(s, keyword_bank(ids + [0], phrases), 0)] + [(NEG, 0, 0)] * (W - 1)
                continue
            c = len(ids) % SENT - 1                                # the content column this step fills
            if bounds is not None and c >= bounds[1]:              # the line is full: PAD alone, as sticky PAD
                cands += [(s, keyword_bank(ids + [0], phrases), 0)] + [(NEG, 0, 0)] * (W - 1)
                continue
            x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V]
            for v in banned_ids(ids, ngram):
                x[v] = float("-inf")
            if bounds is not None and c < bounds[0]:
                x[0] = float("-inf")
            cands += keyword_candidates(x, ids, s, nb, phrases, V)
        if nb > 1:
            gaps.append((len(beams[0][1]), bank_gaps(cands, nb)))
        beams = [(_fork(beams[o // W][0]), beams[o // W][1] + [tok], s) for o, s, _, tok in keyword_select(cands, nb)]
    scores = np.array([s for _, _, s in beams], np.float32)
    met = [keywords_met(ids, phrases) for _, ids, _ in beams]
    order = sorted(sorted(range(nb), key=lambda r: -float(scores[r])), key=lambda r: -met[r])
    return np.array([beams[r][1] for r in order]), scores[order], gaps, np.array([met[r] for r in order])


@functools.lru_cache(maxsize=None)
def fixture_case(case=CASE):
    return setup_case(case)


@functools.lru_cache(maxsize=None)
def cpu_keyword_run(length=FULL, keywords=KEYWORDS, row=ROW, case=CASE):
    """The CPU search the GPU tests compare with (computed once per length)."""
    fx, sh, w, table, batch = fixture_case(case)
    return cpu_keyword_beam_search(w, sh, table, start_row(batch, row), length, NB, keywords, T, REP)


# ------------------------------------------------------------------ 1. entry points
def test_keyword_entry_points_are_declared_exported_bound_and_reject_bad_arguments_without_a_gpu():
    L = hip.lib()
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    names = ("mmtg_decode_beam_candidates_kw", "mmtg_decode_beam_merge_kw", "mmtg_decode_beam_merge_kw_fixed")
    for name in names:
        assert "MMTG_API int %s(" % name in header
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
    # the rhyme form's arguments + phrases, phrase_len, K, phrase_cap, cand_bank; the plain merges' + cand_bank and K
    assert len(hip._SIGS[names[0]][0]) == len(hip._SIGS["mmtg_decode_beam_candidates_rhyme"][0]) + 5
    assert len(hip._SIGS[names[1]][0]) == len(hip._SIGS["mmtg_decode_beam_merge"][0]) + 2
    assert len(hip._SIGS[names[2]][0]) == len(hip._SIGS["mmtg_decode_beam_merge_fixed"][0]) + 2
    assert callable(hip.decode_beam_candidates_kw) and callable(hip.decode_beam_merge_kw) and callable(hip.decode_beam_merge_kw_fixed)
    assert L.mmtg_abi_version() == hip.ABI_VERSION == 12
    p = [0x7000000000 + (i << 24) for i in range(12)]

    def cand(nb=4, K=2, cap=4, bank=p[6], ph=p[7], ln=p[8], cv=p[3]):
        return L.mmtg_decode_beam_candidates_kw(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, nb, cv, p[4], 8, None, 0, None, None,
                                                0, None, 0, None, None, None, None, 0, ph, ln, K, cap, bank, None)

    def merge(nb=4, K=2, bank=p[2], cv=p[3]):                       # (cv: the scores here; None fails the entry's own checks)
        return L.mmtg_decode_beam_merge_kw(p[0], p[1], bank, cv, p[4], 64, p[5], 64, p[6], 64, p[7], 5, SENT, nb, 2, p[8], K, None)

    def fixed(nb=4, K=2, bank=p[2], fe=p[9], cv=p[3]):
        return L.mmtg_decode_beam_merge_kw_fixed(p[0], p[1], bank, cv, p[4], 64, p[5], 64, p[6], 64, p[7], 5, SENT, nb, 2, p[8], fe, K, None)
    for entry, what in ((cand, b"decode_beam_candidates_kw"), (merge, b"decode_beam_merge_kw"), (fixed, b"decode_beam_merge_kw_fixed")):
        for nb in (0, 17):
            assert entry(nb=nb) == -1 and what + b": %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
        for K in (-1, 9):
            assert entry(K=K) == -1 and what + b": %d keywords per prompt (0..8)" % K in L.mmtg_last_error()
        for nb, K in ((16, 1), (13, 7), (15, 3)):                       # 272, 260, 270 candidates
            assert entry(nb=nb, K=K) == -1 and b"candidates exceed the merge workgroup (256)" in L.mmtg_last_error(), (nb, K)
        # 12 x 20 = 240 fits: the call gets past that check and is stopped by the next one (no call here reaches a launch)
        assert entry(nb=12, K=8, cv=None) == -1 and what + b": bad args" in L.mmtg_last_error()
        assert entry(bank=None) == -1 and what in L.mmtg_last_error()
    for cap in (0, 5, -1):
        assert cand(cap=cap) == -1 and b"decode_beam_candidates_kw: phrase length %d outside 1..4" % cap in L.mmtg_last_error()
    assert cand(bank=None) == -1 and b"null cand_bank" in L.mmtg_last_error()
    assert cand(ph=None) == -1 and b"phrases [prompts, 8, 4] and phrase_len [prompts, 8] are needed" in L.mmtg_last_error()
    assert cand(ln=None) == -1 and b"phrases [prompts, 8, 4] and phrase_len [prompts, 8] are needed" in L.mmtg_last_error()
    assert cand(cv=None) == -1 and b"decode_beam_candidates_kw: bad args" in L.mmtg_last_error()
    assert fixed(fe=None) == -1 and b"decode_beam_merge_kw_fixed: null fixed_end" in L.mmtg_last_error()


def test_select_forms_names_the_keyword_entries_on_head_steps_only(monkeypatch):
    from types import SimpleNamespace as NS
    for prefix in (False, True):
        held = "_fixed" if prefix else ""
        for ngram in (0, 3):
            for lines in (False, True):
                was = select_forms(False, prefix, ngram, lines)
                assert select_forms(False, prefix, ngram, lines, keywords=True) == was == (held, held)
                assert select_forms(True, prefix, ngram, lines, keywords=False) == select_forms(True, prefix, ngram, lines)
                assert select_forms(True, prefix, ngram, lines, templates=lines, rhymes=lines, keywords=True) == ("_kw", "_kw" + held)
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
    B, nb, V, K = 8, 4, 160, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                        # noqa: E731
    for with_head in (True, False):
        for prefix in (False, True):
            for kw_on in (False, True):
                fe = i32(B)
                kw = (i32(B // nb, 8, 4), torch.zeros(B // nb, 8, dtype=torch.int8), K, 4) if kw_on else None
                wide = (torch.zeros(B, nb + K), i32(B, nb + K), i32(B, nb + K))
                dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, nb=nb, n_prompts=B // nb,
                         rules=StepRules(prefix=prefix, ngram=3, kw=kw), copy_step=False, fixed_end=fe, logits=torch.zeros(B, V),
                         seq=torch.zeros(B, 64, dtype=torch.long), pos=i32(1), pos_next=i32(1), keep=i32(B, 64), rows=i32(B, 64),
                         scores=torch.zeros(B), cand_val=torch.zeros(B, nb), cand_id=i32(B, nb), params=(1.1, 1.5, 1, 0.0),
                         _kw_cand=wide, _kw_buf=(None, None, None, None))          # (no line tables: the no-leader table is not read)
                held = "_fixed" if prefix else ""
                base = (with_head, 0, dec.params) + (("prefix",) if prefix else ()) + ("ngram", 3)
                assert GreedyDecoder._graph_key(dec, with_head, 0) == base + ((("kw", K), ("cap", 4)) if with_head and kw_on else ())
                del calls[:]
                BeamDecoder._select(dec, with_head)
                if with_head and kw_on:
                    assert [c[0] for c in calls] == ["mmtg_decode_beam_candidates_kw", "mmtg_decode_beam_merge_kw" + held]
                    a = calls[0][1]
                    assert a[11] == wide[0].data_ptr() and a[-6:] == (kw[0].data_ptr(), kw[1].data_ptr(), K, 4, wide[2].data_ptr(), 0)
                    assert a[14:16] == (fe.data_ptr() if prefix else 0, 3) and a[16:26] == (0,) * 10          # no line rule at all
                    m = calls[1][1]
                    assert m[:3] == tuple(t.data_ptr() for t in wide) and m[-2:] == (K, 0) and (not prefix or m[-3] == fe.data_ptr())
                else:                                                  # the entries a search without keywords ends in
                    cand = "_ngram"
                    assert [c[0] for c in calls] == (["mmtg_decode_beam_candidates" + cand] if with_head else []) + ["mmtg_decode_beam_merge" + held]


# ------------------------------------------------------------------ 2. the host checks
def test_check_keywords_packs_and_refuses():
    assert check_keywords(None, 3, 4, 160) is None
    t = check_keywords([(7, 8), [9], (10, 11, 12, 13)], 2, 4, 160)
    assert isinstance(t, KeywordTables) and t.rows == 2 and t.K == 3 and t.cap == 4
    assert t.lists == [((7, 8), (9,), (10, 11, 12, 13))] * 2
    assert t.phrases.dtype == np.int32 and t.phrases.shape == (2, 8, 4) and t.lens.dtype == np.int8 and t.lens.shape == (2, 8)
    assert t.phrases[1, :3].tolist() == [[7, 8, -1, -1], [9, -1, -1, -1], [10, 11, 12, 13]] and (t.phrases[:, 3:] == -1).all()
    assert t.lens.tolist() == [[2, 1, 4, 0, 0, 0, 0, 0]] * 2
    per = check_keywords([[(7, 8)], [(9,), (10,)]], 2, 4, 160)          # one list per prompt; K is the most a prompt has
    assert per.K == 2 and per.lens.tolist() == [[2, 0] + [0] * 6, [1, 1] + [0] * 6] and per.take([1, 1, 0]).lists[2] == ((7, 8),)
    assert check_keywords(per, 2, 4, 160) is per and check_keywords([], 2, 16, 160).K == 0
    assert check_keywords([(i + 10,) for i in range(8)], 1, 8, 160).K == 8                      # 8 x 16 = 128
    bad = [([(7, 0)], "not a content id"), ([(1,)], "not a content id"), ([(2, 7)], "not a content id"), ([(100,)], "not a content id"),
           ([(102,)], "not a content id"), ([(160,)], "not a content id"), ([(-3,)], "not a content id"), ([(7.5,)], "keywords"),
           ([(7, 8, 9, 10, 11)], "1..4 content ids"), ([(7,), ()], "empty phrase|1..4 content ids"),
           ([(7, 8), (7, 8)], "are the same"), ([(7, 8, 9), (8, 9)], "lies inside"), ([(8,), (7, 8, 9)], "lies inside"),
           ([(i + 10,) for i in range(9)], "at most 8"), ("月光", "keywords must be"), ([[(7,)], [(8,)], [(9,)]], "keywords")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            check_keywords(kw, 2, 4, 160)
    with pytest.raises(ValueError, match="below 13317"):
        check_keywords([(13317,)], 1, 4, 21128)
    with pytest.raises(ValueError, match="exceed 256"):
        check_keywords([(7,)], 1, 16, 160)
    assert check_keywords([(i + 10,) for i in range(8)], 1, 9, 160).K == 8                      # 9 x 17 = 153
    with pytest.raises(ValueError, match="exceed 256"):
        check_keywords([(i + 10,) for i in range(8)], 1, 13, 160)                               # 13 x 21 = 273
    with pytest.raises(ValueError, match="keyword tables of 2 prompts"):
        check_keywords(per, 3, 4, 160)
    with pytest.raises(ValueError, match="1..2 content ids"):
        check_keywords([(7, 8, 9)], 1, 4, 160, sent=4)
    # a keyword a given prefix already holds is met from the start (its slot is dead: tests/test_keywords_gpu.py) -- no error
    pre = [[1, 7, 8, 30], [1, 30, 7, 31, 8]]
    t = check_keywords([(7, 8), (30,)], 2, 4, 160, prefix=pre)
    assert keyword_met_mask(pre[0], t.lists[0]) == [True, True] and keyword_met_mask(pre[1], t.lists[1]) == [False, True]
    assert keywords_met(pre[0], t.lists[0]) == 2 and keyword_bank(pre[1], t.lists[1]) == 1
    with pytest.raises(ValueError, match="prefix of 1 rows"):
        check_keywords([(7, 8)], 2, 4, 160, prefix=pre[:1])


class _Tok:
    def convert_tokens_to_ids(self, ch):
        return {"月": 40, "光": 41, "海": 42, "的": 13400, "[": 100}.get(ch, 100)


def test_encode_keywords_and_the_refusals_above_the_decoder():
    assert encode_keywords(_Tok(), ["月光", "海"]) == [(40, 41), (42,)]
    assert encode_keywords(_Tok(), ["的"], vocab_cut=20000) == [(13400,)]
    for words, match in ((["月光", ""], "1..4 characters"), (["月光月光月"], "1..4 characters"), (["月 光"], "not a content id"),
                         (["月亮"], "not a content id"), (["的"], "below 13317"), ("月光", "list of words"), ([40], "1..4 characters")):
        with pytest.raises(ValueError, match=match):
            encode_keywords(_Tok(), words)
    rows = {"topic_ids": np.zeros((1, 5), np.int64)}
    with pytest.raises(ValueError, match="needs beams"):
        generate_samples(_Model(), rows, None, keywords=[(7,)])
    g = GreedyDecoder.__new__(GreedyDecoder)
    with pytest.raises(ValueError, match="needs beams"):
        g.begin({"img_embs": torch.zeros(1, 4)}, 220, keywords=[(7,)])
    with pytest.raises(ValueError, match="needs beams"):
        g.generate({"img_embs": torch.zeros(1, 4)}, 220, keywords=[(7,)])
    dec = BeamDecoder.__new__(BeamDecoder)
    dec.eng = _Eng()
    dec.B, dec.max_len, dec.n_prompts, dec.nb = 4, 220, 1, 4
    one = {"img_embs": torch.zeros(1, 4)}
    for kw, match in ((dict(keywords=[(7,)], num_beam_groups=2, diversity_penalty=0.5), "both allocate the beams"),
                      (dict(keywords=[(7,)], return_logprobs=True), "no return_logprobs"),
                      (dict(keywords=[(7, 0)]), "not a content id"), (dict(keywords=[(7, 8), (8,)]), "lies inside")):
        with pytest.raises(ValueError, match=match):
            dec.begin(one, 220, **kw)
        with pytest.raises(ValueError, match=match):
            dec.generate(one, 220, **kw)
        if "return_logprobs" not in kw:                                # (generate_beams has no return_logprobs to refuse)
            with pytest.raises(ValueError, match=match):
                generate_beams(_Model(), rows, None, num_beams=4, **kw)
    with pytest.raises(ValueError, match="give keywords="):
        dec.generate(one, 220, return_met=True)
    with pytest.raises(ValueError, match="give keywords= and return_all=True"):
        generate_beams(_Model(), rows, None, num_beams=4, keywords=[(7,)], return_met=True)
    dec16 = BeamDecoder.__new__(BeamDecoder)
    dec16.eng = _Eng()
    dec16.B, dec16.max_len, dec16.n_prompts, dec16.nb = 16, 220, 1, 16
    with pytest.raises(ValueError, match="exceed 256"):
        dec16.begin(one, 220, keywords=[(7,)])


# ------------------------------------------------------------------ 3. the bank
def test_keyword_bank_on_hand_written_histories():
    four, two, one = (10, 11, 12, 13), (20, 21), (30,)
    ph = [four, two, one]
    assert keyword_bank([1], ph) == 0 and keyword_bank([1, 50, 51], ph) == 0
    assert keyword_bank([1, 50, 30, 51], ph) == 1 and keyword_bank([1, 20, 21, 50], ph) == 2           # a met phrase counts its length
    assert keyword_bank([1, 10, 11, 12, 13, 50], ph) == 4 and keyword_bank([1, 10, 11, 12, 13, 20, 21, 30], ph) == 7
    assert [keyword_bank([1, 50] + list(four[:m]), ph) for m in (1, 2, 3, 4)] == [1, 2, 3, 4]             # progress 1, 2, 3, then met
    assert keyword_bank([1, 10, 11, 12, 50], ph) == 0 and keyword_bank([1, 10, 11, 50, 12], ph) == 0       # broken: it unwinds
    assert keyword_bank([1, 10, 11, 10], ph) == 1 and keyword_bank([1, 10, 10, 11], ph) == 2               # the longest suffix that is a prefix
    for brk in (0, 2, 1, 100, 102):                                                                     # PAD and the cadence ids break a phrase
        assert keyword_bank([1, 10, 11, brk], ph) == 0 and keyword_bank([1, 10, 11, brk, 12, 13], ph) == 0
        assert keywords_met([1, 10, 11, brk, 12, 13], ph) == 0
    assert keyword_bank([1, 10, 11, 0, 0, 2, 1, 10, 11, 12, 13], ph) == 4                                 # inside one line it is met
    assert keyword_bank([1, 20, 21, 50, 20], ph) == 2 and keyword_bank([1, 30, 30], ph) == 1              # a met keyword gives no progress
    assert keyword_bank([1, 20, 10], ph) == 1 and keyword_bank([1, 10, 11, 12], [four, (12, 40)]) == 3     # two partial phrases: the longer
    assert keyword_bank([1, 10, 11, 12], [(12, 40), four]) == 3 and keyword_bank([1, 12], [(12, 40), four]) == 1
    assert keyword_bank([1, 30, 10, 11], ph) == 1 + 2 and keyword_met_mask([1, 30, 10, 11], ph) == [False, False, True]
    assert keywords_met([1, 10, 11, 12, 13, 20, 21], ph) == 2 and keyword_bank([], ph) == 0 and keyword_bank([1, 5], []) == 0


# ------------------------------------------------------------------ 4. the selection
def _plain_order(cands, nb):
    keyed = [(NEG if np.isnan(np.float32(b)) else np.float32(b), o) for o, (b, _, _) in enumerate(cands)]
    return [o for _, o in sorted(keyed, key=lambda c: (-float(c[0]), c[1]))[:nb]]


def test_keyword_select_is_the_rule():
    rng = np.random.RandomState(3)
    for nb, K in ((4, 3), (6, 2), (8, 8), (16, 0)):
        W = nb + K
        base = (-rng.rand(nb * W) * 4).astype(np.float32)
        base[rng.rand(nb * W) < 0.2] = NEG
        base[5] = np.float32("nan")
        base[7] = base[9] = np.float32(-1.25)                       # an exact tie: the lower o first
        toks = rng.randint(3, 99, nb * W)
        for same in (0, 3):                                           # with all banks equal: the plain (score, parent, rank) order
            kept = keyword_select([(b, same, t) for b, t in zip(base, toks)], nb)
            assert [c[0] for c in kept] == _plain_order([(b, same, t) for b, t in zip(base, toks)], nb)
            assert all(c[1].tobytes() == (NEG if np.isnan(base[c[0]]) else base[c[0]]).tobytes() and c[3] == toks[c[0]] for c in kept)
        banks = rng.randint(0, 7, nb * W)
        cands = list(zip(base, banks, toks))
        kept = keyword_select(cands, nb)
        live = [o for o in range(nb * W) if base[o] > NEG]
        assert 5 not in [c[0] for c in kept[:len(live)]]             # NaN is dead
        tops = {}                                                     # the best of each bank, highest bank first
        for o in live:
            if banks[o] not in tops or (base[o], -o) > (base[tops[banks[o]]], -tops[banks[o]]):
                tops[banks[o]] = o
        want = [tops[k] for k in sorted(tops, reverse=True)]
        n = min(nb, len(want))
        assert [c[0] for c in kept[:n]] == want[:n] and [c[2] for c in kept[:n]] == sorted(tops, reverse=True)[:n]
        if nb > len(want):                                            # then the second best of each bank that has one
            second = [max((o for o in live if banks[o] == k and o != tops[k]), key=lambda o: (base[o], -o), default=None)
                      for k in sorted(tops, reverse=True)]
            second = [o for o in second if o is not None]
            m = min(nb - len(want), len(second))
            assert [c[0] for c in kept[len(want):len(want) + m]] == second[:m]
    # dead candidates come last, in o order, and only when the live ones run out
    cands = [(NEG, 5, 1), (np.float32(-1.0), 0, 2), (np.float32("nan"), 6, 3), (np.float32(-2.0), 2, 4), (NEG, 0, 5)]
    assert [c[0] for c in keyword_select(cands, 4)] == [3, 1, 0, 2]
    assert [float(c[1]) for c in keyword_select(cands, 4)] == [-2.0, -1.0, float("-inf"), float("-inf")]


# ------------------------------------------------------------------ 5. the CPU search
def test_keywords_are_still_found_under_ngram_bans_and_line_bounds():
    """What tests/test_keywords_gpu.py relies on when it combines keywords with no_repeat_ngram_size=3 and line_lengths=(3, 18):
    for prompt 0 the CPU search under the same constraints returns a first hypothesis with both keywords, over a run without a
    near-tie, and breaks neither constraint."""
    fx, sh, w, table, batch = fixture_case()
    ids, scores, gaps, met = cpu_keyword_beam_search(w, sh, table, start_row(batch, 0), FULL, NB, KEYWORDS, T, REP, ngram=3, bounds=(3, 18))
    assert met[0] == 2 and comparable_length(gaps, FULL) == FULL
    for r in ids.tolist():
        assert all(r[c] not in banned_ids(r[:c], 3) for c in range(1, len(r)))
        for line in _content_lines(r)[:FULL // SENT]:
            k = sum(1 for v in line if v != 0)
            assert 3 <= k <= 18 and all(v != 0 for v in line[:k])


def _content_lines(row):
    return [row[s + 1:s + SENT - 1] for s in range(0, len(row), SENT)]


def test_without_keywords_the_cpu_search_is_the_plain_one():
    fx, sh, w, table, batch = fixture_case()
    for row, length in ((0, 44), (2, 30)):
        ids, scores, gaps = cpu_beam_search(w, sh, table, start_row(batch, row), length, NB, T, REP)
        kids, kscores, kgaps, met = cpu_keyword_beam_search(w, sh, table, start_row(batch, row), length, NB, [], T, REP)
        assert kids.tolist() == ids.tolist() and kscores.tobytes() == scores.tobytes() and met.tolist() == [0] * NB
        assert comparable_length(kgaps, length, tol=0.0) == length and len(kgaps) == len(gaps)


def test_keywords_the_plain_search_leaves_out_are_found_by_the_constrained_one():
    """The fixture cannot make this vacuous: the plain four-beam search of the prompt holds neither keyword in any hypothesis, the
    constrained one returns a first hypothesis with both.  Its score is the sum of the processed log-probabilities of its free
    columns (recomputed here by teacher forcing on the oracle), no phrase spans a line, and the run the GPU test compares over is at
    least two lines long with a keyword completed inside it."""
    fx, sh, w, table, batch = fixture_case()
    start = start_row(batch, ROW)
    assert len(KEYWORDS) == 2 and sorted(len(p) for p in KEYWORDS) == [1, 2]
    assert check_keywords(list(KEYWORDS), 1, NB, sh.V).K == 2
    plain, _, _ = cpu_beam_search(w, sh, table, start, FULL, NB, T, REP)
    assert all(keywords_met(r, KEYWORDS) == 0 for r in plain.tolist())
    ids, scores, gaps, met = cpu_keyword_run()
    assert ids.shape == (NB, 1 + FULL) and met[0] == 2 and keywords_met(ids[0].tolist(), KEYWORDS) == 2
    assert (np.diff(met) <= 0).all() and all(scores[i] >= scores[i + 1] for i in range(NB - 1) if met[i] == met[i + 1])
    assert len({tuple(r) for r in ids.tolist()}) == NB and np.isfinite(scores).all()
    for j in range(2, 1 + FULL):                                     # the cadence, on every beam
        if (j + 1) % SENT in (0, 1):
            assert (ids[:, j] == (2 if (j + 1) % SENT == 0 else 1)).all()
    best = ids[0].tolist()
    for p in KEYWORDS:                                               # every phrase lies inside one line
        assert any(tuple(line[i:i + len(p)]) == p for line in _content_lines(best) for i in range(len(line)))
    # the score: teacher forcing on the oracle, the processed log-probability of every free column the model chose
    base = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in start.items()}
    base["topic_ids"] = base["topic_ids"].long()
    cf, total = O.CachedForward(w, sh, table), 0.0
    for i in range(FULL):
        if i > 0 and (i + 2) % SENT in (0, 1):
            continue
        logits = cf(dict(base, targets=torch.tensor([best[:i + 1]], dtype=torch.long)))[0, -1, :]
        if best[i] == 0:
            continue
        x = O.process_logits(logits, torch.tensor(best[:i + 1]), T, REP)[:min(sh.V, 13317)]
        total += float(torch.log_softmax(x, -1)[best[i + 1]])
    np.testing.assert_allclose(float(scores[0]), total, rtol=1e-5)
    # the condition of the GPU comparison, from the CPU search alone
    L = comparable_length(gaps, FULL)
    print("comparable run", L, "min gap", min(g for _, g in gaps))
    assert L >= 2 * SENT
    assert keywords_met(ids[0, :1 + L].tolist(), KEYWORDS) >= 1
