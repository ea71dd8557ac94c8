"""Prefixed generation (GreedyDecoder / BeamDecoder with prefix=..., generate_samples / generate_beams with prefixes=...) on the host:
encode_prefix against the reference dataset layout, the prefix rules, the new ABI entries' argument checks, and the CPU restatement
of prefixed decoding that tests/test_prefix_gpu.py holds the decoder to.

The restatement runs the oracle (oracle.mmtg_oracle.CachedForward, process_logits) with the forced [#EOS#] / [#START#] cadence on
the ABSOLUTE lyric column, the slot layout of the training data.  For a whole-line prefix that is the reference loop
sample_sequence(targets=prefix, length - (L - 1)) exactly, and for a prefix cut from the reference's own greedy output it returns that
output -- the check of the yardstick against the reference."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from mmtg_amd import hip
from mmtg_amd.data import encode_prefix
from mmtg_amd.decode import GreedyDecoder, check_prefix
from oracle import mmtg_oracle as O
from test_beam_cpu import NEG, SENT, _fork, setup_case, start_row
from test_data_cpu import FixtureTokenizer

T, REP = 1.1, 1.5


# ------------------------------------------------------------------ the CPU restatements
def _base(start):
    base = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in start.items() if k not in ("targets", "rating")}
    base["topic_ids"] = base["topic_ids"].long()
    return base


def cpu_prefixed_greedy(w, sh, table, start, prefix, length, temperature=T, repetition_penalty=REP):
    """Greedy decoding of one prompt from `prefix`: the 1 + length lyric columns, column c < L the prefix, every later column by
    the absolute slot cadence (c % SENT == SENT - 1: [#EOS#], c % SENT == 0: [#START#]), sticky PAD, or the arg-max of the
    processed logits (the penalty counts the prefix), cut at 13317."""
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
        x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V]
        ids.append(int(torch.argmax(x).item()))
    return ids


def cpu_prefixed_beam_search(w, sh, table, start, prefix, length, nb, temperature=T, repetition_penalty=REP):
    """test_beam_cpu.cpu_beam_search started from `prefix` with the absolute slot cadence: every beam holds the prefix, the prefix
    positions add nothing to a score.  Returns (ids [nb, 1 + length] best first, scores [nb] fp32, gaps) as cpu_beam_search."""
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
            x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V]
            lp = torch.log_softmax(x, -1)
            order = torch.sort(x, descending=True, stable=True).indices[:nb]
            cands += [(np.float32(s + np.float32(lp[v].item())), q, k, int(v)) for k, v in enumerate(order.tolist())]
        cands.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
        if len(cands) > nb:
            gaps.append((c, float(cands[nb - 1][0]) - float(cands[nb][0])))
        beams = [(_fork(beams[q][0]), beams[q][1] + [tok], s) for s, q, _, tok in cands[:nb]]
    return np.array([ids for _, ids, _ in beams]), np.array([s for _, _, s in beams], np.float32), gaps


def golden_prefix(fx, row, k):
    """The first k lines (+ the next [#START#]) of the reference's own greedy output for prompt `row` of a fixture."""
    return fx["greedy_len220_row%d" % row][:1 + SENT * k].tolist()


# ------------------------------------------------------------------ encode_prefix
@pytest.fixture(scope="module")
def dataset_fixture():
    fx = np.load(os.path.join(GOLDEN, "dataset.npz"))
    meta = json.loads(str(fx["meta_json"]))
    return fx, meta


def test_encode_prefix_is_the_dataset_layout(dataset_fixture):
    """Whole lines give the first 22 k + 1 ids of the reference dataset's targets (the next line's [#START#] included); a partial
    line adds its words unpadded."""
    fx, meta = dataset_fixture
    tok = FixtureTokenizer(meta)
    for n in range(2):
        lyrics = meta["records"][n]["lyrics"]
        targets = fx["item%d_targets" % n].tolist()
        for k in range(1, 5):
            got = encode_prefix(tok, lyrics[:k])
            assert got == targets[:SENT * k + 1], (n, k)
            check_prefix([got], 1, 220)
            part = encode_prefix(tok, lyrics[:k], partial=lyrics[k])
            words = [v for v in targets[SENT * k + 1:SENT * (k + 1) - 1] if v != 0]
            assert part == targets[:SENT * k + 1] + words, (n, k)
            check_prefix([part], 1, 220)
        assert encode_prefix(tok, []) == [1]
        assert encode_prefix(tok, [], partial=lyrics[0]) == targets[:1] + [v for v in targets[1:SENT - 1] if v != 0]


# ------------------------------------------------------------------ the prefix rules
def test_check_prefix_accepts_both_forms_and_rejects_invalid_prefixes():
    line = [1] + [30] * 5 + [0] * 15 + [2]
    good = [[1], line + [1], line + [1, 40, 41], line + line + [1], line + [1, 40, 0]]
    assert check_prefix(good, 5, 220) == good
    a = torch.full((5, 46), -1, dtype=torch.long)
    for b, p in enumerate(good):
        a[b, :len(p)] = torch.tensor(p)
    assert check_prefix(a, 5, 220) == good
    assert check_prefix(a.numpy(), 5, 220) == good
    bad = {
        "rows": ([[1]] * 3, 2, 220),
        "empty": ([[]], 1, 220),
        "start": ([[2, 30]], 1, 220),
        "next start": ([line + [30]], 1, 220),
        "eos": ([line[:-1] + [30]], 1, 220),
        "banned 1": ([[1, 1]], 1, 220),
        "banned 2": ([[1, 30, 2]], 1, 220),
        "banned 100": ([[1, 100]], 1, 220),
        "banned 102": ([[1, 102]], 1, 220),
        "negative": ([[1, -5]], 1, 220),
        "vocabulary": ([[1, 160]], 1, 220),
        "too long": ([line + [1]], 1, 21),
        "gap in padding": (torch.tensor([[1, -1, 30]]), 1, 220),
        "not 2-D": (torch.tensor([1, 30]), 1, 220),
    }
    for name, (p, rows, length) in bad.items():
        with pytest.raises(ValueError):
            check_prefix(p, rows, length, V=160)
            pytest.fail(name)
    check_prefix([line + [1]], 1, 22)                    # L = length + 1: the whole output is the prefix


# ------------------------------------------------------------------ the ABI entries
def test_prefix_entry_points_are_exported_and_reject_bad_arguments_without_a_gpu():
    L = hip.lib()
    names = ("mmtg_decode_select_fixed", "mmtg_decode_sample_fixed", "mmtg_decode_beam_candidates_fixed", "mmtg_decode_beam_merge_fixed")
    for name in names:
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
    p = [0x7000000000 + (i << 24) for i in range(10)]
    rc = L.mmtg_decode_select_fixed(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, None)
    assert rc == -1 and b"decode_select_fixed: null fixed_end" in L.mmtg_last_error()
    rc = L.mmtg_decode_select_fixed(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[2], p[4], None)
    assert rc == -1 and b"decode_select_fixed: pos_next must not alias pos_ptr" in L.mmtg_last_error()
    rc = L.mmtg_decode_sample_fixed(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[5], 8, 8, p[3], None, None)
    assert rc == -1 and b"decode_sample_fixed: null fixed_end" in L.mmtg_last_error()
    rc = L.mmtg_decode_sample_fixed(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, None, 8, 8, p[3], p[4], None)
    assert rc == -1 and b"decode_sample_fixed: uniforms" in L.mmtg_last_error()
    rc = L.mmtg_decode_beam_candidates_fixed(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[3], p[4], 8, None, None)
    assert rc == -1 and b"decode_beam_candidates_fixed: null fixed_end" in L.mmtg_last_error()
    rc = L.mmtg_decode_beam_merge_fixed(p[0], p[1], p[2], p[3], 64, p[4], 64, p[5], 64, p[6], 5, SENT, 4, 2, p[7], None, None)
    assert rc == -1 and b"decode_beam_merge_fixed: null fixed_end" in L.mmtg_last_error()
    for nb in (0, 17):
        rc = L.mmtg_decode_beam_candidates_fixed(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, nb, p[3], p[4], 8, p[5], None)
        assert rc == -1 and b"decode_beam_candidates_fixed: %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
        rc = L.mmtg_decode_beam_merge_fixed(p[0], p[1], p[2], p[3], 64, p[4], 64, p[5], 64, p[6], 5, SENT, nb, 2, p[7], p[8], None)
        assert rc == -1 and b"decode_beam_merge_fixed: %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
    # the Python wrappers check the prefix-end array before the library sees it
    with pytest.raises(ValueError, match="fixed_end"):
        hip._fixed(torch.zeros(4, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="fixed_end"):
        hip._fixed(torch.zeros(3, dtype=torch.int32), 4)


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("row,k", [(0, 1), (1, 2), (2, 4)])
def test_restatement_is_the_reference_loop_for_whole_line_prefixes(row, k):
    """A whole-line prefix (a prompt's own dataset lines): the restatement's reference_return cut equals the oracle's
    sample_sequence(targets=prefix, length - (L - 1))."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    start = start_row(batch, row)
    prefix = batch["targets"][row, :1 + SENT * k].tolist()
    length = 120
    ids = cpu_prefixed_greedy(w, sh, table, start, prefix, length)
    assert ids[:len(prefix)] == prefix and len(ids) == 1 + length
    ref = O.sample_sequence(O.CachedForward(w, sh, table), dict(start, targets=np.asarray(prefix)), length - (len(prefix) - 1),
                            temperature=T, top_k=1, top_p=0.0, repitition_penalty=REP, greedy=True)
    assert GreedyDecoder.reference_return(ids, length) == ref


@pytest.mark.parametrize("row,k", [(0, 1), (0, 3), (1, 1), (1, 9)])
def test_restatement_returns_the_reference_greedy_output_from_its_own_lines(row, k):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ids = cpu_prefixed_greedy(w, sh, table, start_row(batch, row), golden_prefix(fx, row, k), 220)
    assert GreedyDecoder.reference_return(ids, 220) == fx["greedy_len220_row%d" % row].tolist()


def test_restatement_partial_line_keeps_the_absolute_cadence():
    """A partial-line prefix: the line is completed in its own slot ([#EOS#] at the slot's last column, not 20 tokens after the
    prefix as the reference loop would place it) and every rule holds."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    prefix = batch["targets"][0, :SENT + 4].tolist()
    assert 0 not in prefix[SENT + 1:]
    ids = cpu_prefixed_greedy(w, sh, table, start_row(batch, 0), prefix, 88)
    assert ids[:len(prefix)] == prefix
    for c in range(1, 89):
        if c % SENT == SENT - 1:
            assert ids[c] == 2
        elif c % SENT == 0:
            assert ids[c] == 1
        else:
            assert ids[c] not in (1, 2, 100, 102)
            if c >= len(prefix) and ids[c - 1] == 0:
                assert ids[c] == 0


def test_prefixed_beam_search_at_one_beam_is_the_prefixed_greedy_restatement():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    start = start_row(batch, 1)
    prefix = golden_prefix(fx, 1, 2)
    ids, scores, _ = cpu_prefixed_beam_search(w, sh, table, start, prefix, 100, 1)
    assert ids[0].tolist() == cpu_prefixed_greedy(w, sh, table, start, prefix, 100)
    assert np.isfinite(scores[0]) and scores[0] < 0
    ids4, scores4, _ = cpu_prefixed_beam_search(w, sh, table, start, prefix, 100, 4)
    assert (ids4[:, :len(prefix)] == np.asarray(prefix)).all() and len({tuple(r) for r in ids4.tolist()}) == 4
    assert (np.diff(scores4) <= 0).all()
