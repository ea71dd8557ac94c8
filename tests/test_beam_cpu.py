"""Beam search (mmtg_amd.decode.BeamDecoder): the host side of its ABI and the CPU beam search that pins it.

The reference (src/generate.py) has no beam search, so no golden file can pin the feature.  `cpu_beam_search` below restates it on
the committed oracle (oracle.mmtg_oracle.CachedForward, process_logits, fp32 log_softmax); at one beam it must be the oracle's own
greedy sample_sequence -- the check on the yardstick itself.  tests/test_beam_gpu.py holds the decoder to it."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from helpers import batch_to_torch, load_case
from mmtg_amd import hip
from mmtg_amd.decode import GreedyDecoder
from oracle import mmtg_oracle as O

SENT = 22
NEG = np.float32(-np.inf)


def _fork(cf):
    c = copy.copy(cf)
    c.k, c.v = list(cf.k), list(cf.v)
    return c


def cpu_beam_search(w, sh, table, start, length, nb, temperature, repetition_penalty):
    """One prompt (`start`: a dataset row without targets), `nb` beams, the reference loop's cadence (generate.py:117-142).
    Returns (ids [nb, 1 + length] best first, scores [nb] fp32, gaps): gaps[c] = (lyric column appended by model call c, the gap
    between the nb-th and (nb+1)-th candidate of that selection)."""
    base = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in start.items() if k not in ("targets", "rating")}
    base["topic_ids"] = base["topic_ids"].long()
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    cf0 = O.CachedForward(w, sh, table)
    beams = [(cf0, [1], np.float32(0.0))] + [(_fork(cf0), [1], NEG) for _ in range(nb - 1)]
    gaps = []
    for i in range(length):
        if i > 0 and (i + 2) % SENT in (0, 1):                     # forced [#EOS#] / [#START#]: every beam, score unchanged
            tok = 2 if (i + 2) % SENT == 0 else 1
            beams = [(cf, ids + [tok], s) for cf, ids, s in beams]
            continue
        cands = []                                                 # (score, parent, rank, token)
        for p, (cf, ids, s) in enumerate(beams):
            if s == NEG:                                           # a start beam: its candidates are all -inf
                cands += [(NEG, p, k, 0) for k in range(nb)]
                continue
            inputs = dict(base, targets=torch.tensor([ids], dtype=torch.long))
            logits = cf(inputs)[0, -1, :]
            if ids[-1] == 0:                                       # sticky PAD: one candidate, the score unchanged
                cands += [(s, p, 0, 0)] + [(NEG, p, k, 0) for k in range(1, nb)]
                continue
            x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V]
            lp = torch.log_softmax(x, -1)
            order = torch.sort(x, descending=True, stable=True).indices[:nb]
            cands += [(np.float32(s + np.float32(lp[v].item())), p, k, int(v)) for k, v in enumerate(order.tolist())]
        cands.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
        if len(cands) > nb:
            gaps.append((len(beams[0][1]), float(cands[nb - 1][0]) - float(cands[nb][0])))
        beams = [(_fork(beams[p][0]), beams[p][1] + [tok], s) for s, p, _, tok in cands[:nb]]
    return np.array([ids for _, ids, _ in beams]), np.array([s for _, _, s in beams], np.float32), gaps


def comparable_length(gaps, length, tol=1e-4):
    """Generated columns up to (not including) the first selection whose nb-th / (nb+1)-th gap is below `tol` (finite gaps only):
    two fp32 searches that differ in the last bits may order that selection differently."""
    for col, gap in gaps:
        if np.isfinite(gap) and gap < tol:
            return col - 1
    return length


def setup_case(name):
    fx, meta, mcfg, gcfg, dcfg, weights, table, batch = load_case(name)
    sh = O.Shapes(mcfg, dcfg, gcfg)
    return fx, sh, O.weights_to_torch(weights), torch.from_numpy(table), batch_to_torch(batch)


def start_row(batch, row):
    return {k: v[row].numpy() for k, v in batch.items() if k not in ("rating", "targets")}


def test_beam_entry_points_load_and_reject_bad_beam_counts_without_a_gpu():
    """The new ABI entries resolve, and nb outside 1..16 is rejected on the host with the library's message before any device
    call (as test_host_cpu.py's round-4 checks)."""
    L = hip.lib()
    for name in ("mmtg_decode_attn_split_rows", "mmtg_decode_attn_split_x3_rows", "mmtg_decode_beam_candidates", "mmtg_decode_beam_merge"):
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
    p = [0x7000000000 + (i << 24) for i in range(10)]
    for nb in (0, 17):
        rc = L.mmtg_decode_beam_candidates(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, nb, p[3], p[4], 8, None)
        assert rc == -1 and b"decode_beam_candidates: %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
        rc = L.mmtg_decode_beam_merge(p[0], p[1], p[2], p[3], 64, p[4], 64, p[5], 64, p[6], 5, SENT, nb, 2, p[7], None)
        assert rc == -1 and b"decode_beam_merge: %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
    # the table-aware attention refuses a table narrower than the cache
    rc = L.mmtg_decode_attn_split_rows(hip.BF16, p[0], 2, p[1], p[2], p[3], p[4], 64, p[5], 32, p[6], p[7], 8, 12, 64, 64, None)
    assert rc == -1 and b"decode_attn_split_rows" in L.mmtg_last_error()
    rc = L.mmtg_decode_attn_split_x3_rows(p[0], 2, p[1], p[2], p[3], p[4], 64, p[5], 32, p[6], p[7], 8 * 12 * 64, 8, 12, 64, 64, None)
    assert rc == -1 and b"decode_attn_split_x3_rows" in L.mmtg_last_error()


def test_beam_decoder_rejects_bad_settings_without_a_gpu():
    from mmtg_amd.decode import BeamDecoder
    for nb in (0, 17):
        with pytest.raises(ValueError, match="num_beams"):
            BeamDecoder(None, 2, nb)
    with pytest.raises(ValueError, match="one lane"):
        BeamDecoder(None, 2, 4, lanes=2)


@pytest.mark.parametrize("row", [0, 1, 2])
def test_cpu_beam_search_at_one_beam_is_the_oracle_greedy_loop(row):
    """The yardstick: one beam of the CPU search picks what the oracle's greedy sample_sequence picks (rank rule 3: the
    processed logit, then the id -- not the rounded log-probability)."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    start = start_row(batch, row)
    length = 220 if row == 0 else 60
    ids, scores, _ = cpu_beam_search(w, sh, table, start, length, 1, 1.1, 1.5)
    got = GreedyDecoder.reference_return(ids[0].tolist(), length)
    st = dict(start, targets=np.asarray([1]))
    ref = O.sample_sequence(O.CachedForward(w, sh, table), st, length, temperature=1.1, top_k=1, top_p=0.0, repitition_penalty=1.5,
                            greedy=True)
    assert got == ref
    key = "greedy_len%d_row%d" % (length, row)
    if key in fx.files:
        assert got == fx[key].tolist()
    assert np.isfinite(scores[0]) and scores[0] < 0


@pytest.mark.parametrize("case", ["tiny_s5", "tiny_lstm2_rnn2"])
def test_cpu_beam_search_rules_and_comparable_length(case):
    """Four beams: the forced cadence on every beam, scores sorted best first, no duplicate hypotheses -- and the fixtures and
    length tests/test_beam_gpu.py compares at keep at least 60 generated positions of some prompt before its first near-tie
    selection (measured here: tiny_s5 37 / 9 / 120, tiny_lstm2_rnn2 120 / 120 / 120 of 120)."""
    fx, sh, w, table, batch = setup_case(case)
    length = 120
    lens = []
    for row in range(batch["topic_ids"].shape[0]):
        ids, scores, gaps = cpu_beam_search(w, sh, table, start_row(batch, row), length, 4, 1.1, 1.5)
        assert ids.shape == (4, 1 + length) and (ids[:, 0] == 1).all()
        assert np.isfinite(scores).all() and (np.diff(scores) <= 0).all()
        assert len({tuple(r) for r in ids.tolist()}) == 4                     # no duplicate hypotheses
        for j in range(2, 1 + length):
            if (j + 1) % SENT == 0:
                assert (ids[:, j] == 2).all()
            elif (j + 1) % SENT == 1:
                assert (ids[:, j] == 1).all()
        lens.append(comparable_length(gaps, length))
    assert max(lens) >= 60, lens
