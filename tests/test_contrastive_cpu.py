"""Contrastive search (mmtg_amd.decode.ContrastiveDecoder): the host side of its two ABI entries, the host checks, and the CPU
contrastive search that pins it.

The reference (src/generate.py) has no contrastive search, so no golden file can pin the feature.  `cpu_contrastive_search` below
restates the rule of include/mmtg_hip.h on the committed oracle (a CachedForward that also keeps the ln_f output of the last
position, process_logits, fp32 log_softmax, the cadence and sticky PAD of tests/test_beam_cpu.py's cpu_beam_search); at alpha = 0
and at top_k = 1 it must be the oracle's own greedy sample_sequence -- the check on the yardstick itself.
tests/test_contrastive_gpu.py holds the decoder to it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.constraints import check_contrastive
from mmtg_amd.decode import ContrastiveDecoder, GreedyDecoder
from oracle import mmtg_oracle as O
from test_beam_cpu import NEG, SENT, _fork, comparable_length, setup_case, start_row

T, REP = 1.1, 1.5
# the settings tests/test_contrastive_gpu.py follows the CPU search at, per fixture: (top_k, penalty_alpha, length).  The usual
# alpha = 0.6, k = 4 does not meet the two conditions of test_cpu_contrastive_search_leaves_the_greedy_path on these fixtures: their
# random weights give nearly uniform probabilities and nearly equal cosines, so most choices are made by less than 1e-4 (comparable
# lengths 31 / 23 / 10 with one non-top pick on tiny_s5; 19 / 39 / 7 with one at alpha 0.5 on tiny_lstm2_rnn2).  A sweep of the CPU
# search alone over alpha in 0.1 .. 0.9 and k in {2, 3, 4, 8} gave the settings below: tiny_s5 comparable lengths 16 / 9 / 94 with
# 0 / 3 / 8 non-top picks inside them, tiny_lstm2_rnn2 120 / 15 / 4 with 5 / 0 / 0.
FOLLOW = {"tiny_s5": (4, 0.9, 120), "tiny_lstm2_rnn2": (3, 0.8, 120)}


class HiddenForward(O.CachedForward):
    """CachedForward that also keeps `hidden`: the ln_f output of the last position of the call (the last layer_norm the forward
    runs), fp32 [D].  The logits are the base class's, bit for bit."""

    def __call__(self, batch):
        seen, orig = [], O.layer_norm

        def spy(*a, **kw):
            out = orig(*a, **kw)
            seen.append(out)
            return out

        O.layer_norm = spy
        try:
            logits = super().__call__(batch)
        finally:
            O.layer_norm = orig
        self.hidden = seen[-1][0, -1].float()
        return logits


def cpu_contrastive_search(w, sh, table, start, length, k, alpha, temperature, repetition_penalty, prefix=None):
    """One prompt (`start`: a dataset row without targets).  Token step `col` runs the model on every live candidate of lyric column
    col, keeps r* = argmax (1 - alpha) * exp(score) - alpha * sim (fp32; the lowest r on a tie; sim = the largest dot of the
    candidate's unit ln_f state with those of the kept lyric columns before it, 0 for none) and offers column col + 1: a prefix id,
    the forced cadence token, a sticky PAD -- each by row 0 alone at score 0 -- or the top k of the chosen row's processed logits.
    Returns a list of one record per step: col, tok (the chosen token), r (r*), gap (best minus second-best contrastive score, inf
    with one live candidate), total (the fp32 sum of the chosen scores so far) and top (token, score): the first candidate of
    column col + 1.  ``truncate`` turns the records into the ids and the score of a generation of any length up to `length`."""
    base = {k_: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k_, v in start.items() if k_ not in ("targets", "rating")}
    base["topic_ids"] = base["topic_ids"].long()
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    a32 = np.float32(alpha)
    cf = HiddenForward(w, sh, table)
    ids, ctx, rec = [], [], []
    total = np.float32(0.0)
    cands = [(1 if prefix is None else int(prefix[0]), np.float32(0.0))]
    with torch.no_grad():
        for col in range(length):
            live = []
            for r, (tok, s) in enumerate(cands):
                if s == NEG:
                    continue
                c = _fork(cf)
                logits = c(dict(base, targets=torch.tensor([ids + [tok]], dtype=torch.long)))[0, -1, :]
                nrm = torch.sqrt((c.hidden * c.hidden).sum())
                u = c.hidden / nrm if float(nrm) > 0 else torch.zeros_like(c.hidden)
                sims = [np.float32(torch.dot(u, cu).item()) for cu, kp in ctx if kp]
                sim = max(sims) if sims else np.float32(0.0)
                cs = np.float32(np.float32(np.float32(1.0) - a32) * np.exp(np.float32(s))) - np.float32(a32 * sim)
                live.append((cs, r, tok, s, c, logits, u))
            best = max(live, key=lambda e: (float(e[0]), -e[1]))
            others = sorted((float(e[0]) for e in live if e is not best), reverse=True)
            gap = float(best[0]) - others[0] if others else float("inf")
            _, r_star, tok, s, cf, logits, u = best
            ids.append(tok)
            ctx.append((u, tok != 0))
            total = np.float32(total + s)
            j = col + 1
            if prefix is not None and j < len(prefix):
                cands = [(int(prefix[j]), np.float32(0.0))]
            elif j > 1 and (j + 1) % SENT == 0:
                cands = [(2, np.float32(0.0))]
            elif j > 1 and (j + 1) % SENT == 1:
                cands = [(1, np.float32(0.0))]
            elif tok == 0:                                             # sticky PAD, the score unchanged
                cands = [(0, np.float32(0.0))]
            else:
                x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V]
                lp = torch.log_softmax(x, -1)
                order = torch.sort(x, descending=True, stable=True).indices[:k]
                cands = [(int(v), np.float32(lp[v].item())) for v in order.tolist()]
                cands = [(v, s_) if np.isfinite(s_) else (0, NEG) for v, s_ in cands]
            rec.append(dict(col=col, tok=tok, r=r_star, gap=gap, total=total, top=cands[0]))
    return rec


def truncate(rec, length):
    """(ids [1 + length], score) of the generation of `length` steps: the chosen tokens of columns 0 .. length - 1, then the most
    probable candidate of column `length`, which no step judges."""
    last = rec[length - 1]
    return [e["tok"] for e in rec[:length]] + [last["top"][0]], np.float32(last["total"] + last["top"][1])


def comparable(rec, length):
    """tests/test_beam_cpu.py's comparable_length over the contrastive gaps: the generation length up to which two fp32 searches
    must agree (every choice before it was made by more than 1e-4)."""
    return comparable_length([(e["col"], e["gap"]) for e in rec], length)


@functools.lru_cache(maxsize=None)
def follow_runs(case):
    """The CPU search of every prompt of fixture `case` at FOLLOW's settings, run once and shared (the GPU tests read it too)."""
    k, alpha, length = FOLLOW[case]
    fx, sh, w, table, batch = setup_case(case)
    return [cpu_contrastive_search(w, sh, table, start_row(batch, row), length, k, alpha, T, REP)
            for row in range(batch["topic_ids"].shape[0])]


def _greedy_reference(w, sh, table, start, length):
    st = dict(start, targets=np.asarray([1]))
    return O.sample_sequence(O.CachedForward(w, sh, table), st, length, temperature=T, top_k=1, top_p=0.0, repitition_penalty=REP, greedy=True)


def test_contrastive_entry_points_load_and_reject_bad_arguments_without_a_gpu():
    """The two new ABI entries resolve, and k = 0, k = 17, alpha < 0, alpha > 1, aliasing position slots and the similarity entry's
    own bad sizes are rejected on the host with the library's message before any device call."""
    L = hip.lib()
    for name in ("mmtg_decode_contrastive_sim", "mmtg_decode_contrastive_merge"):
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
    p = [0x7000000000 + (i << 24) for i in range(12)]

    def merge(k=4, alpha=0.6, pos_next=p[9], scores=p[2]):
        return L.mmtg_decode_contrastive_merge(p[0], p[1], scores, p[3], p[4], alpha, p[5], 64, p[6], 64, p[7], 64, p[8], 5, SENT, k, 2,
                                               pos_next, None, None)

    for k in (0, 17):
        assert merge(k=k) == -1 and b"decode_contrastive_merge: top_k %d outside 1..16" % k in L.mmtg_last_error()
    for alpha in (-0.01, 1.01, float("nan")):
        assert merge(alpha=alpha) == -1 and b"decode_contrastive_merge: penalty_alpha" in L.mmtg_last_error()
    assert merge(pos_next=p[8]) == -1 and b"decode_contrastive_merge: pos_next must not alias pos_ptr" in L.mmtg_last_error()
    assert merge(scores=None) == -1 and b"decode_contrastive_merge: null pointer" in L.mmtg_last_error()

    def sim(D=768, x=p[0], hc_len=8, ldkeep=64, dtype=hip.F32):
        return L.mmtg_decode_contrastive_sim(dtype, x, D, p[1], p[2], 1e-5, p[3], hc_len, p[4], p[5], p[6], ldkeep, p[7], 64, p[8], 5, 8, D,
                                             None)

    for D in (0, 770, 1028):
        assert sim(D=D) == -1 and b"decode_contrastive_sim: n_embd %d" % D in L.mmtg_last_error()
    assert sim(x=None) == -1 and b"decode_contrastive_sim: null pointer" in L.mmtg_last_error()
    assert sim(hc_len=0) == -1 and b"decode_contrastive_sim: bad sizes" in L.mmtg_last_error()
    assert sim(ldkeep=5) == -1 and b"decode_contrastive_sim: bad sizes" in L.mmtg_last_error()
    assert sim(dtype=7) == -1 and b"decode_contrastive_sim: bad dtype 7" in L.mmtg_last_error()


def test_contrastive_host_checks_raise_before_device_work():
    assert check_contrastive(4, 0.6) == (4, 0.6) and check_contrastive(np.int64(1), 0) == (1, 0.0) and check_contrastive(16, 1) == (16, 1.0)
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="top_k"):
            check_contrastive(k, 0.6)
    for k in (2.0, "4", True, None):
        with pytest.raises(ValueError, match="top_k must be an integer"):
            check_contrastive(k, 0.6)
    for a in (-0.1, 1.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="penalty_alpha"):
            check_contrastive(4, a)
    # the decoder: a bad top_k before the model is touched; what the method does not take, with the reason
    for k in (0, 17):
        with pytest.raises(ValueError, match="top_k"):
            ContrastiveDecoder(None, 2, k)
    with pytest.raises(ValueError, match="one lane"):
        ContrastiveDecoder(None, 2, 4, lanes=2)
    with pytest.raises(ValueError, match="no keywords=.*one hypothesis"):
        ContrastiveDecoder._refuse(keywords=[(5, 6)])
    with pytest.raises(ValueError, match="num_beam_groups.*not beams"):
        ContrastiveDecoder._refuse(num_beam_groups=2)
    with pytest.raises(ValueError, match="return_logprobs.*score_sequences"):
        ContrastiveDecoder._refuse(return_logprobs=True)
    with pytest.raises(ValueError, match="diversity_penalty.*no beam groups"):
        ContrastiveDecoder._refuse(diversity_penalty=1.0)
    for kw in (dict(top_k=10), dict(top_p=0.7), dict(generator=object())):
        with pytest.raises(ValueError, match="deterministic.*sampling"):
            ContrastiveDecoder._refuse(**kw)
    ContrastiveDecoder._refuse()
    from mmtg_amd.generate import generate_contrastive
    with pytest.raises(ValueError, match="keywords"):
        generate_contrastive(None, [], None, keywords=[(5, 6)])
    with pytest.raises(ValueError, match="num_beam_groups"):
        generate_contrastive(None, [], None, num_beam_groups=2)
    with pytest.raises(ValueError, match="penalty_alpha"):
        generate_contrastive(None, [], None, penalty_alpha=2.0)


@pytest.mark.parametrize("k,alpha,row,length", [(4, 0.0, 0, 220), (3, 0.0, 1, 60), (1, 0.6, 0, 220), (1, 1.0, 2, 60)])
def test_cpu_contrastive_search_without_a_penalty_or_a_choice_is_the_oracle_greedy_loop(k, alpha, row, length):
    """The yardstick: at alpha = 0 (any k) and at top_k = 1 (any alpha) the CPU search picks what the oracle's greedy
    sample_sequence picks, and never leaves candidate 0."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    start = start_row(batch, row)
    rec = cpu_contrastive_search(w, sh, table, start, length, k, alpha, T, REP)
    ids, score = truncate(rec, length)
    assert GreedyDecoder.reference_return(ids, length) == _greedy_reference(w, sh, table, start, length)
    assert all(e["r"] == 0 for e in rec)
    assert np.isfinite(score) and score < 0
    key = "greedy_len%d_row%d" % (length, row)
    if key in fx.files:
        assert GreedyDecoder.reference_return(ids, length) == fx[key].tolist()


@pytest.mark.parametrize("case", sorted(FOLLOW))
def test_cpu_contrastive_search_leaves_the_greedy_path(case):
    """At FOLLOW's settings, on every fixture the GPU test follows: the forced cadence, a finite score -- and inside the columns
    before the first choice made by less than 1e-4 (comparable_length) the search picks a candidate other than the most probable
    one at least 3 times over the fixture's prompts, those columns numbering at least 40 on some prompt.  (FOLLOW states the measured
    values.)"""
    k, alpha, length = FOLLOW[case]
    fx, sh, w, table, batch = setup_case(case)
    lens, picks = [], 0
    for row, rec in enumerate(follow_runs(case)):
        ids, score = truncate(rec, length)
        assert len(ids) == 1 + length and ids[0] == 1 and np.isfinite(score) and score < 0
        for j in range(2, 1 + length):
            if (j + 1) % SENT == 0:
                assert ids[j] == 2
            elif (j + 1) % SENT == 1:
                assert ids[j] == 1
            else:
                assert ids[j] not in (1, 2, 100, 102) and (ids[j - 1] != 0 or ids[j] == 0)
        L = comparable(rec, length)
        lens.append(L)
        picks += sum(1 for e in rec[:L] if e["r"] != 0)
    print(case, "comparable lengths", lens, "non-top picks inside them", picks)
    assert picks >= 3, (lens, picks)
    assert max(lens) >= 40, lens


def test_cpu_contrastive_search_holds_a_prefix():
    """A given opening comes back unchanged, chosen by row 0 alone at score 0, and the search goes on from it."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    pre = [1] + list(range(30, 50)) + [2, 1, 60, 61, 62]
    rec = cpu_contrastive_search(w, sh, table, start_row(batch, 0), 60, 4, 0.6, T, REP, prefix=pre)
    ids, score = truncate(rec, 60)
    assert ids[:len(pre)] == pre and all(e["r"] == 0 and e["gap"] == float("inf") for e in rec[:len(pre)])
    assert float(rec[len(pre) - 1]["total"]) == 0.0 and np.isfinite(score) and score < 0
