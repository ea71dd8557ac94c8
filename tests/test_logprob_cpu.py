"""Token log-probabilities on the host: which columns count towards a row's score (decode.chosen_mask / sequence_scores) on
hand-written rows, the ranking behind generate_samples(rank_by=), and the new ABI entry's declaration, export and argument checks."""
import ctypes
import os

import numpy as np
import pytest

from mmtg_amd import hip
from mmtg_amd.decode import chosen_mask, sequence_scores
from mmtg_amd.generate import rank_scored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(content, sent):
    """[#START#], the content ids padded with PAD to sent - 2 columns, [#EOS#]."""
    return [1] + list(content) + [0] * (sent - 2 - len(content)) + [2]


# ------------------------------------------------------------------ the mask
def test_chosen_mask_counts_content_and_the_first_pad_of_a_line_sent_22():
    sent = 22
    full = list(range(10, 30))                                                # a full line: 20 content ids, no PAD
    ids = [line(full, sent) + line([40, 41], sent) + [1, 50],                 # a line that pads from its third token; a partial line
           line([], sent) + line([60], sent) + [1, 0]]                        # an empty line; one token; an empty partial line
    m = chosen_mask(ids, sent=sent)
    assert m.shape == (2, 46) and m.dtype == bool
    for b in range(2):
        assert not m[b, [0, 21, 22, 43, 44]].any()                            # column 0 and the cadence columns never count
    assert m[0, 1:21].all()                                                   # every token of the full line
    assert m[0, 23:26].tolist() == [True, True, True] and not m[0, 26:43].any()   # 40, 41, the FIRST pad; the sticky ones do not count
    assert m[0, 45]
    assert m[1, 1] and not m[1, 2:21].any()                                   # an empty line: its first content column alone
    assert m[1, 23:25].tolist() == [True, True] and not m[1, 25:43].any()
    assert m[1, 45]                                                           # the PAD that opens the last line (after [#START#])
    assert m.sum(1).tolist() == [24, 4]


def test_chosen_mask_sent_6_prefix_and_upto():
    sent = 6
    row = line([7, 8, 9, 3], sent) + line([5, 0, 0, 0], sent) + line([0, 0, 0, 0], sent) + [1]
    ids = np.array([row, row, row])
    m = chosen_mask(ids, sent=sent, prefix_lens=[0, 3, 8])                    # no prefix; one that ends mid-line; one past line 0
    want0 = [j for j in range(19) if j % 6 not in (0, 5) and row[j - 1] != 0]
    assert want0 == [1, 2, 3, 4, 7, 8, 13]
    assert np.flatnonzero(m[0]).tolist() == want0
    assert np.flatnonzero(m[1]).tolist() == [3, 4, 7, 8, 13]                  # columns 0 .. 2 were given
    assert np.flatnonzero(m[2]).tolist() == [8, 13]                           # column 7 was given, column 8 is the line's first PAD
    assert np.array_equal(chosen_mask(ids, sent=sent), np.stack([m[0]] * 3))
    lp = -np.arange(19, dtype=np.float32)[None, :].repeat(3, 0)               # column j holds -j
    s, c = sequence_scores(ids, lp, sent=sent, prefix_lens=[0, 3, 8])
    assert s.dtype == np.float64 and s.tolist() == [-38.0, -35.0, -21.0] and c.tolist() == [7, 5, 2]
    s, c = sequence_scores(ids, lp, sent=sent, prefix_lens=[0, 3, 8], upto=8)     # the columns below 8
    assert s.tolist() == [-17.0, -14.0, 0.0] and c.tolist() == [5, 3, 0]
    s, c = sequence_scores(ids, lp, sent=sent, upto=0)
    assert s.tolist() == [0.0] * 3 and c.tolist() == [0] * 3
    lp[0, 6] = -np.inf                                                        # a column that does not count may hold anything
    lp[1, 7] = -np.inf                                                        # one that counts makes the sum -inf
    s, _ = sequence_scores(ids, lp, sent=sent)
    assert s[0] == -38.0 and s[1] == -np.inf
    with pytest.raises(ValueError):
        sequence_scores(ids, lp[:, :5], sent=sent)
    with pytest.raises(ValueError):
        chosen_mask(ids, sent=sent, prefix_lens=[0, 1])
    with pytest.raises(ValueError):
        chosen_mask(row, sent=sent)


# ------------------------------------------------------------------ the ranking
def test_rank_scored_is_stable_and_mean_survives_zero_tokens():
    scored = [("a", -6.0, 3), ("b", -4.0, 1), ("c", -6.0, 6), ("d", 0.0, 0), ("e", -4.0, 4), ("f", -4.0, 1)]
    assert [t[0] for t in rank_scored(scored, "sum")] == ["d", "b", "e", "f", "a", "c"]      # ties keep their draw order
    # means: a -2, b -4, c -1, d 0 / max(0, 1) = 0, e -1, f -4
    assert [t[0] for t in rank_scored(scored, "mean")] == ["d", "c", "e", "a", "b", "f"]
    assert rank_scored([], "mean") == []
    assert [t[0] for t in rank_scored([("x", -np.inf, 2), ("y", -1.0, 2)], "mean")] == ["y", "x"]
    for bad in ("best", "", 1):
        with pytest.raises(ValueError):
            rank_scored(scored, bad)
    assert scored[0] == ("a", -6.0, 3)                                        # the input list is left alone


# ------------------------------------------------------------------ ABI
def test_logprob_entry_is_declared_exported_bound_and_rejects_bad_arguments_without_a_gpu():
    lib = hip.lib()
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    exports = open(os.path.join(ROOT, "mmtg_amd", "csrc", "exports.map")).read()
    name = "mmtg_decode_logprob"
    assert "MMTG_API int %s(" % name in header
    assert "global: mmtg_*;" in exports                                       # the export list is the mmtg_ prefix
    assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
    assert len(hip._SIGS[name][0]) == 12 and callable(hip.decode_logprob)
    p = [0x7000000000 + (i << 24) for i in range(4)]
    ok = dict(logits=p[0], ldl=168, V=160, seq=p[1], ldseq=64, pos=p[2], P=5, out=p[3], ldo=45, ncols=45, B=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mmtg_decode_logprob(a["logits"], a["ldl"], a["V"], a["seq"], a["ldseq"], a["pos"], a["P"], a["out"], a["ldo"], a["ncols"],
                                       a["B"], None)
    for k in ("logits", "seq", "pos", "out"):
        assert call(**{k: None}) == -1 and b"decode_logprob: null pointer" in lib.mmtg_last_error()
    for kw in (dict(B=0), dict(V=0), dict(ldl=159), dict(P=-1), dict(ldseq=5), dict(ncols=0), dict(ldo=44)):
        assert call(**kw) == -1, kw
        assert b"decode_logprob: logits [B, ldl >= V]" in lib.mmtg_last_error()
    import torch
    with pytest.raises(ValueError, match="out must be fp32"):
        hip.decode_logprob(None, 168, 160, torch.zeros(8, 64, dtype=torch.long), None, 5, torch.zeros(8, 45, dtype=torch.float64), 8)
