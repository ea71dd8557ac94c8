"""n-gram blocking (no_repeat_ngram_size) on the host: a restatement of the ban rule of include/mmtg_hip.h checked on hand-written
histories, check_ngram, the new ABI entries' argument checks, and the CPU restatements of greedy decoding and beam search with bans
that tests/test_ngram_gpu.py holds the decoder to.

The restatements are those of tests/test_prefix_cpu.py (the oracle's CachedForward and process_logits, the absolute slot cadence)
with the banned ids' processed logits set to -inf before the arg-max / the log_softmax.  With n = 0 they are the reference loop."""
import ctypes

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_ngram
from oracle import mmtg_oracle as O
from test_beam_cpu import NEG, SENT, _fork, setup_case, start_row
from test_prefix_cpu import REP, T, _base

NONCONTENT = (0, 1, 2, 100, 102)         # PAD, [#START#], [#EOS#], [UNK], [SEP]


# ------------------------------------------------------------------ the rule
def content(v):
    return int(v) not in NONCONTENT


def banned_ids(g, n):
    """The ids row history g (its lyric columns before the one it fills) may not write next with no_repeat_ngram_size n."""
    g = [int(v) for v in g]
    j = len(g)
    if n < 1 or j < n - 1:
        return set()
    key = g[j - n + 1:]
    if not all(content(v) for v in key):
        return set()
    return {g[i + n - 1] for i in range(j - n + 1) if all(content(v) for v in g[i:i + n]) and g[i:i + n - 1] == key}


def violations(ids, n, start=1):
    """Columns c >= start whose id is banned by ids[:c] (forced and PAD columns never are: a banned id is content)."""
    ids = [int(v) for v in ids]
    return [c for c in range(start, len(ids)) if n > 0 and ids[c] in banned_ids(ids[:c], n)]


def repeated_ngrams(ids, n):
    """Content n-grams of ids that occur more than once (the rule's converse: none after a generation with size n)."""
    seen, rep = set(), set()
    for i in range(len(ids) - n + 1):
        w = tuple(int(v) for v in ids[i:i + n])
        if all(content(v) for v in w):
            (rep if w in seen else seen).add(w)
    return rep


def test_ban_rule_on_hand_written_histories():
    line = [1, 30, 31, 32, 0, 0]
    # n = 1: every content id already held; PAD and the specials never
    assert banned_ids([1, 30, 31, 0, 30, 2, 1], 1) == {30, 31}
    assert banned_ids([], 1) == set() and banned_ids([1], 1) == set()
    # n = 2: the key is the last id; a non-content key bans nothing
    assert banned_ids([1, 30, 31, 30], 2) == {31}
    assert banned_ids([1, 30, 31, 30, 32, 30], 2) == {31, 32}
    for cut in (0, 1, 2):                               # PAD, [#START#], [#EOS#] as the key: nothing banned
        assert banned_ids([1, 30, 31, cut], 2) == set()
    # n = 3: keys cut by PAD / [#START#] / [#EOS#] never match across them
    assert banned_ids([1, 30, 31, 33, 30, 31], 3) == {33}
    assert banned_ids([1, 30, 0, 31, 5, 30, 0], 3) == set()
    assert banned_ids([1, 30, 31, 2, 1, 30, 31], 3) == set()                # (30, 31) ended by [#EOS#]: no content 3-gram
    assert banned_ids([1, 30, 31, 40, 2, 1, 30, 31], 3) == {40}             # ... but (30, 31, 40) is one
    assert banned_ids([1, 30, 31, 2, 1, 31], 3) == set()                     # a key crossing [#START#] is not all content
    # a repeated whole line: the copy is blocked at its n-th content column
    hist = line + [1, 30, 31]
    assert banned_ids(hist, 3) == {32} and banned_ids(hist, 4) == set() and banned_ids(hist + [32], 4) == set()
    # a history shorter than n - 1
    assert banned_ids([1, 30], 4) == set() and banned_ids([30, 31], 3) == set()
    assert banned_ids([30, 31, 30], 3) == set() and banned_ids([30, 31, 30, 31], 3) == {30}
    # overlapping matches: 30 30 30 bans 30 for n = 2 and n = 3, every window counts
    assert banned_ids([1, 30, 30, 30], 3) == {30}
    assert banned_ids([1, 30, 30, 30, 31, 30, 30], 3) == {30, 31}
    assert banned_ids([1, 30, 31, 30, 31, 30], 3) == {31}
    assert violations([1, 30, 31, 30, 31], 2) == [4] and violations([1, 30, 31, 30, 32], 2) == []
    assert repeated_ngrams([1, 30, 31, 30, 31], 2) == {(30, 31)}


def test_check_ngram_accepts_the_range_and_rejects_the_rest():
    for sent in (22, 7):
        for n in range(sent - 1):
            assert check_ngram(n, sent) == n and type(check_ngram(np.int64(n), sent)) is int
        for bad in (-1, sent - 1, 100, 2.0, 3.5, "3", None, True, False, np.bool_(True), [2]):
            with pytest.raises(ValueError):
                check_ngram(bad, sent)
    assert check_ngram(20) == 20


class _Sh:
    msl, max_seq_length, V = 20, 220, 160


class _Eng:
    sh = _Sh()

    @property
    def dev(self):
        raise AssertionError("device work before the validation")


class _Model:
    def engine(self):
        return _Eng()


def test_generate_entry_points_validate_before_any_device_work():
    from mmtg_amd.generate import generate_beams, generate_samples
    rows = {"topic_ids": np.zeros((1, 5), np.int64)}
    for bad in (21, -1, 2.5, True):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            generate_samples(_Model(), rows, None, no_repeat_ngram_size=bad)
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            generate_beams(_Model(), rows, None, no_repeat_ngram_size=bad)


def test_ngram_entry_points_are_exported_and_reject_bad_arguments_without_a_gpu():
    L = hip.lib()
    for name in ("mmtg_decode_select_ngram", "mmtg_decode_sample_ngram", "mmtg_decode_beam_candidates_ngram"):
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
    p = [0x7000000000 + (i << 24) for i in range(10)]
    for n in (0, -1, SENT - 1, 1000):
        rc = L.mmtg_decode_select_ngram(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, n, None)
        assert rc == -1 and b"decode_select_ngram: n-gram size %d outside 1..20" % n in L.mmtg_last_error()
        rc = L.mmtg_decode_sample_ngram(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[5], 8, 8, p[3], p[4], n, None)
        assert rc == -1 and b"decode_sample_ngram: n-gram size %d outside 1..20" % n in L.mmtg_last_error()
        rc = L.mmtg_decode_beam_candidates_ngram(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[3], p[4], 8, None, n, None)
        assert rc == -1 and b"decode_beam_candidates_ngram: n-gram size %d outside 1..20" % n in L.mmtg_last_error()
    rc = L.mmtg_decode_select_ngram(p[0], 160, 160, p[1], 64, p[2], 5, 7, 1.1, 1.5, 8, p[3], None, 6, None)
    assert rc == -1 and b"n-gram size 6 outside 1..5" in L.mmtg_last_error()
    rc = L.mmtg_decode_select_ngram(None, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, 3, None)
    assert rc == -1 and b"decode_select_ngram: the n-gram form needs logits" in L.mmtg_last_error()
    rc = L.mmtg_decode_select_ngram(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[2], None, 3, None)
    assert rc == -1 and b"decode_select_ngram: pos_next must not alias pos_ptr" in L.mmtg_last_error()
    rc = L.mmtg_decode_select_ngram(p[0], 40000, 40000, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], p[4], 3, None)
    assert rc == -1 and b"decode_select_ngram: vocabulary of 40000" in L.mmtg_last_error()
    rc = L.mmtg_decode_sample_ngram(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, None, 8, 8, p[3], None, 3, None)
    assert rc == -1 and b"decode_sample_ngram: uniforms" in L.mmtg_last_error()
    rc = L.mmtg_decode_sample_ngram(p[0], 30000, 30000, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[5], 8, 8, p[3], None, 3, None)
    assert rc == -1 and b"decode_sample_ngram: vocabulary of 30000" in L.mmtg_last_error()
    for nb in (0, 17):
        rc = L.mmtg_decode_beam_candidates_ngram(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, nb, p[3], p[4], 8, p[5], 3, None)
        assert rc == -1 and b"decode_beam_candidates_ngram: %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
    rc = L.mmtg_decode_beam_candidates_ngram(p[0], 30000, 30000, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[3], p[4], 8, None, 3, None)
    assert rc == -1 and b"decode_beam_candidates_ngram: vocabulary of 30000" in L.mmtg_last_error()


def test_decoders_reject_a_bad_ngram_size_before_any_device_work():
    for cls in (GreedyDecoder, BeamDecoder):
        dec = cls.__new__(cls)
        dec.eng = _Eng()
        dec.B, dec.max_len, dec.n_prompts, dec.nb = 1, 220, 1, 1
        batch = {"img_embs": torch.zeros(1, 4)}
        for bad in (21, -2, 1.0, False):
            with pytest.raises(ValueError, match="no_repeat_ngram_size"):
                dec.begin(batch, 30, no_repeat_ngram_size=bad)


# ------------------------------------------------------------------ the CPU restatements
def cpu_ngram_greedy(w, sh, table, start, length, n, prefix=(1,), temperature=T, repetition_penalty=REP):
    """test_prefix_cpu.cpu_prefixed_greedy with the ids banned by no_repeat_ngram_size n set to -inf in the processed logits."""
    base = _base(start)
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    cf = O.CachedForward(w, sh, table)
    ids = [int(v) for v in prefix]
    for c in range(len(ids), length + 1):
        if c % SENT == SENT - 1:
            ids.append(2)
            continue
        if c % SENT == 0:
            ids.append(1)
            continue
        logits = cf(dict(base, targets=torch.tensor([ids], dtype=torch.long)))[0, -1, :]
        if ids[-1] == 0:
            ids.append(0)
            continue
        x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V].clone()
        for v in banned_ids(ids, n):
            x[v] = float("-inf")
        ids.append(int(torch.argmax(x).item()))
    return ids


def cpu_ngram_beam_search(w, sh, table, start, length, nb, n, prefix=(1,), temperature=T, repetition_penalty=REP):
    """test_prefix_cpu.cpu_prefixed_beam_search with each beam's banned ids (on its own history) at -inf before the log_softmax and
    the top nb.  Returns (ids [nb, 1 + length] best first, scores [nb] fp32, gaps)."""
    base = _base(start)
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    cf0 = O.CachedForward(w, sh, table)
    p = [int(v) for v in prefix]
    beams = [(cf0, list(p), np.float32(0.0))] + [(_fork(cf0), list(p), NEG) for _ in range(nb - 1)]
    gaps = []
    for c in range(len(p), length + 1):
        if c % SENT in (0, SENT - 1):
            tok = 2 if c % SENT == SENT - 1 else 1
            beams = [(cf, ids + [tok], s) for cf, ids, s in beams]
            continue
        cands = []
        for q, (cf, ids, s) in enumerate(beams):
            if s == NEG:
                cands += [(NEG, q, k, 0) for k in range(nb)]
                continue
            logits = cf(dict(base, targets=torch.tensor([ids], dtype=torch.long)))[0, -1, :]
            if ids[-1] == 0:
                cands += [(s, q, 0, 0)] + [(NEG, q, k, 0) for k in range(1, nb)]
                continue
            x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V].clone()
            for v in banned_ids(ids, n):
                x[v] = float("-inf")
            lp = torch.log_softmax(x, -1)
            order = torch.sort(x, descending=True, stable=True).indices[:nb]
            for k, v in enumerate(order.tolist()):
                ok = bool(torch.isfinite(x[v]))
                cands.append((np.float32(s + np.float32(lp[v].item())) if ok else NEG, q, k, int(v) if ok else 0))
        cands.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
        if len(cands) > nb:
            gaps.append((c, float(cands[nb - 1][0]) - float(cands[nb][0])))
        beams = [(_fork(beams[q][0]), beams[q][1] + [tok], s) for s, q, _, tok in cands[:nb]]
    return np.array([ids for _, ids, _ in beams]), np.array([s for _, _, s in beams], np.float32), gaps


def first_repeat(ids, n):
    """The first column whose id completes a content n-gram held earlier (None: no such column)."""
    v = violations(ids, n)
    return v[0] if v else None


@pytest.mark.parametrize("row", [0, 1])
def test_restatement_obeys_the_rule_and_leaves_repeat_free_output_alone(row):
    """n = 3 on tiny_s5 (its greedy outputs repeat content bigrams but no 3-gram): the reference output comes back unchanged;
    n = 0 is the reference output itself."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row%d" % row].tolist()
    assert repeated_ngrams(ref, 2) and not repeated_ngrams(ref, 3)
    start = start_row(batch, row)
    assert GreedyDecoder.reference_return(cpu_ngram_greedy(w, sh, table, start, 220, 0), 220) == ref
    ids = cpu_ngram_greedy(w, sh, table, start, 220, 3)
    assert GreedyDecoder.reference_return(ids, 220) == ref and not violations(ids, 3)


@pytest.mark.parametrize("row", [0, 1])
def test_restatement_with_bigram_bans_departs_at_the_first_repeated_bigram(row):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row%d" % row].tolist()
    c = first_repeat(ref, 2)
    assert c is not None
    ids = cpu_ngram_greedy(w, sh, table, start_row(batch, row), 220, 2)
    assert ids[:c] == ref[:c] and ids[c] != ref[c]
    assert not violations(ids, 2) and not repeated_ngrams(ids, 2)
    one = cpu_ngram_greedy(w, sh, table, start_row(batch, row), 100, 1)
    assert not violations(one, 1) and not repeated_ngrams(one, 1)


def test_beam_restatement_obeys_the_rule_and_one_beam_is_greedy():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    start = start_row(batch, 1)
    for n in (1, 2):
        ids1, s1, _ = cpu_ngram_beam_search(w, sh, table, start, 90, 1, n)
        assert ids1[0].tolist() == cpu_ngram_greedy(w, sh, table, start, 90, n)
        ids, scores, _ = cpu_ngram_beam_search(w, sh, table, start, 90, 4, n)
        assert np.isfinite(scores).all() and (np.diff(scores) <= 0).all()
        assert len({tuple(r) for r in ids.tolist()}) == 4
        for r in ids.tolist():
            assert not violations(r, n), n
    prefix = fx["greedy_len220_row1"][:1 + SENT].tolist()
    ids, _, _ = cpu_ngram_beam_search(w, sh, table, start, 70, 4, 2, prefix=prefix)
    for r in ids.tolist():
        assert r[:len(prefix)] == prefix and not violations(r, 2, start=len(prefix))
