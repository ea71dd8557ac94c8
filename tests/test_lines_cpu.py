"""Line-length bounds and line-end token sets (line_lengths= / line_end_ids=) on the host: a restatement of the rule of
include/mmtg_hip.h checked on hand-written columns, check_lines, the new ABI entries' argument checks, and the CPU restatements of
greedy decoding and beam search under the rule that tests/test_lines_gpu.py holds the decoder to.

The restatements are those of tests/test_ngram_cpu.py (the oracle's CachedForward and process_logits, the absolute slot cadence, the
n-gram bans) with the rule's bans set to -inf in the processed logits before the arg-max / the log_softmax, and a full line writing
PAD without a look at the logits.  With unconstrained tables they are the reference loop."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, LineTables, check_lines
from oracle import mmtg_oracle as O
from test_beam_cpu import NEG, SENT, _fork, setup_case, start_row
from test_ngram_cpu import _Eng, _Model, banned_ids
from test_prefix_cpu import REP, T, _base

CAP = SENT - 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the rule
def line_rule(g, lo, hi, ends, sent=SENT):
    """What the rule says of the free column a row with history g (its lyric columns so far) fills next, on a line with bounds
    lo, hi and end set ends (None: no set): "pad" (the line is full: PAD, no logits), or (pad_banned, allowed) with allowed the
    set the content ids are confined to (None: all)."""
    j = len(g)
    c = j % sent - 1
    assert 0 <= c <= sent - 3, "a forced column"
    if c >= hi:
        return "pad"
    pad_banned = c < lo or (ends is not None and int(g[-1]) not in ends)
    return pad_banned, (ends if ends is not None and c == hi - 1 else None)


def apply_rule(x, g, lo, hi, ends, sent=SENT):
    """The processed logits x [V] of the column after history g under the rule (None: the line is full, the row writes PAD)."""
    r = line_rule(g, lo, hi, ends, sent)
    if r == "pad":
        return None
    pad_banned, allowed = r
    x = x.clone()
    if allowed is not None:
        keep = torch.zeros_like(x, dtype=torch.bool)
        keep[sorted(allowed)] = True
        keep[0] = True                                     # PAD stays subject to its own rule
        x[~keep] = float("-inf")
    if pad_banned:
        x[0] = float("-inf")
    return x


def line_lengths_of(ids, sent=SENT):
    """Content tokens (not PAD) per whole line of a row of lyric ids [1 + length]."""
    ids = [int(v) for v in ids]
    return [sum(1 for v in ids[l * sent + 1:l * sent + sent - 1] if v != 0) for l in range(len(ids) // sent)]


def rule_violations(ids, tables, b, start=1, n=0, sent=SENT):
    """Columns c >= start of row ids that break the rule of tables' row b given the columns before them: every chosen column is
    checked (forced columns against the cadence), none skipped.  A sticky-PAD column must be PAD; a full line's column must be
    PAD; PAD where it is banned and a content id outside a confining end set are violations unless every id was banned (only
    n-gram bans can empty a set: then PAD is what the kernels write)."""
    ids = [int(v) for v in ids]
    bad = []
    for c in range(start, len(ids)):
        q = c % sent
        if q == 0 or q == sent - 1:
            if ids[c] != (1 if q == 0 else 2):
                bad.append(c)
            continue
        if ids[c - 1] == 0:
            if ids[c] != 0:
                bad.append(c)
            continue
        lo, hi, ends = tables.bounds(b, c // sent)
        r = line_rule(ids[:c], lo, hi, ends, sent)
        if r == "pad":
            if ids[c] != 0:
                bad.append(c)
            continue
        pad_banned, allowed = r
        if ids[c] == 0:
            emptied = allowed is not None and n > 0 and set(allowed) <= banned_ids(ids[:c], n)
            if pad_banned and not emptied:
                bad.append(c)
        elif allowed is not None and ids[c] not in allowed:
            bad.append(c)
    return bad


def test_rule_on_hand_written_columns():
    ends = {30, 31}
    # bounds alone: PAD banned below lo, free between, the line full at hi
    assert line_rule([1], 2, 4, None) == (True, None) and line_rule([1, 40], 2, 4, None) == (True, None)
    assert line_rule([1, 40, 41], 2, 4, None) == (False, None) and line_rule([1, 40, 41, 42], 2, 4, None) == (False, None)
    assert line_rule([1, 40, 41, 42, 43], 2, 4, None) == "pad"
    assert line_rule([1], 0, 0, None) == "pad" and line_rule([1], 0, CAP, None) == (False, None)
    # hi = sent - 2 never fills: column sent - 3 is the last content column
    assert line_rule([1] + [40] * (CAP - 1), 0, CAP, None) == (False, None)
    # an end set: PAD only after a member, never at c = 0 ([#START#] is no member), the last column confined to the set
    assert line_rule([1], 0, 3, ends) == (True, None)
    assert line_rule([1, 40], 0, 3, ends) == (True, None) and line_rule([1, 30], 0, 3, ends) == (False, None)
    assert line_rule([1, 40, 41], 0, 3, ends) == (True, ends) and line_rule([1, 40, 31], 0, 3, ends) == (False, ends)
    assert line_rule([1, 40, 41, 30], 0, 3, ends) == "pad"
    assert line_rule([1, 30], 2, 3, ends) == (True, None)                    # a member below lo: PAD still banned
    assert line_rule([1], 1, 1, ends) == (True, ends)                        # a one-token line is a member
    # the second line of a row: the column counts from its own [#START#]
    first = [1] + [40] * 3 + [0] * (CAP - 3) + [2]
    assert line_rule(first + [1, 40], 2, 2, None) == (True, None) and line_rule(first + [1, 40, 41], 2, 2, None) == "pad"
    x = torch.arange(64, dtype=torch.float32)
    y = apply_rule(x, [1, 40, 41], 0, 3, ends)
    assert torch.isfinite(y).nonzero().flatten().tolist() == [30, 31] and torch.equal(y[30:32], x[30:32])
    y = apply_rule(x, [1, 40, 31], 0, 3, ends)
    assert torch.isfinite(y).nonzero().flatten().tolist() == [0, 30, 31]
    y = apply_rule(x, [1], 2, 5, None)
    assert torch.isinf(y[0]) and torch.equal(y[1:], x[1:])
    assert apply_rule(x, [1, 40], 0, 1, None) is None
    assert torch.equal(apply_rule(x, [1, 40], 0, CAP, None), x)
    t = check_lines([2, (1, 3)], [None, ends], 1, 2 * SENT, SENT, 64)
    ok = [1, 40, 41] + [0] * (CAP - 2) + [2, 1, 40, 30] + [0] * (CAP - 2) + [2, 1]
    assert rule_violations(ok, t, 0) == [] and line_lengths_of(ok) == [2, 2]
    assert rule_violations(ok[:2] + [0] * (CAP - 1) + ok[SENT - 1:], t, 0) == [2]              # PAD below lo
    assert rule_violations(ok[:3] + [42] + ok[4:], t, 0) == [3]                                # content in a full line
    assert rule_violations(ok[:SENT + 2] + [41] + ok[SENT + 3:], t, 0) == [SENT + 3]           # PAD after a non-member
    assert rule_violations(ok[:SENT + 2] + [41, 42] + ok[SENT + 4:], t, 0) == [SENT + 3]       # a non-member in the last column


# ------------------------------------------------------------------ check_lines
def test_check_lines_packs_every_accepted_form():
    assert check_lines(None, None, 3, 220, SENT, 160) is None
    t = check_lines(7, None, 3, 220, SENT, 160)
    assert isinstance(t, LineTables) and t.lo.shape == (3, 10) and t.lo.dtype == np.uint8 and t.hi.dtype == np.uint8
    assert (t.lo == 7).all() and (t.hi == 7).all() and t.sets is None and t.set_of is None
    t = check_lines((1, CAP), None, 2, 44, SENT, 160)
    assert t.lo.tolist() == [[1, 1]] * 2 and t.hi.tolist() == [[CAP, CAP]] * 2
    t = check_lines([5, None, (0, 3), np.int64(4)], None, 2, 220, SENT, 160)
    assert t.lo[1].tolist() == [5, 0, 0, 4] + [0] * 6 and t.hi[0].tolist() == [5, CAP, 3, 4] + [CAP] * 6
    t = check_lines([[5, 6], None, (2, 3)], None, 3, 44, SENT, 160)              # one list, None or entry per row
    assert t.lo.tolist() == [[5, 6], [0, 0], [2, 2]] and t.hi.tolist() == [[5, 6], [CAP, CAP], [3, 3]]
    t = check_lines(None, [None, {30, 31}, None, [31, 30], (40,)], 2, 220, SENT, 160)
    assert t.set_of.dtype == np.int16 and t.set_of[0].tolist() == [-1, 0, -1, 0, 1] + [-1] * 5 and t.set_of[1].tolist() == t.set_of[0].tolist()
    assert t.sets.dtype == np.uint32 and t.sets.shape == (2, 5) and (t.lo == 0).all() and (t.hi == CAP).all()
    assert t.bounds(0, 1) == (0, CAP, frozenset({30, 31})) and t.bounds(1, 4)[2] == frozenset({40}) and t.bounds(0, 0)[2] is None
    assert t.bounds(0, 99) == (0, CAP, None)
    assert int(t.sets[0, 0]) == (1 << 30) | (1 << 31) and int(t.sets[1, 1]) == 1 << 8
    t = check_lines(3, frozenset({30}), 2, 44, SENT, 160)                          # one set for every line
    assert t.set_of.tolist() == [[0, 0]] * 2
    t = check_lines(None, [[None, {30}], None, [[31, 32]]], 3, 44, SENT, 160)     # per row
    assert t.set_of.tolist() == [[-1, 0], [-1, -1], [1, -1]]
    r = t.repeat(2)
    assert r.rows == 6 and r.set_of.tolist() == [[-1, 0]] * 2 + [[-1, -1]] * 2 + [[1, -1]] * 2 and r.sets is t.sets
    assert check_lines([None], None, 1, 1, SENT, 160).lo.shape == (1, 1)
    assert check_lines(3, None, 1, SENT + 1, SENT, 160).lo.shape == (1, 2) and check_lines(3, None, 1, SENT, SENT, 160).lo.shape == (1, 1)
    # a partial prefix line within its hi
    pre = [[1] + [40] * CAP + [2, 1, 41, 42]]
    assert check_lines([None, (0, 2)], None, 1, 60, SENT, 160, prefix=pre) is not None
    assert check_lines([1, 5], None, 1, 60, SENT, 160, prefix=pre) is not None    # whole given lines are not checked


@pytest.mark.parametrize("lens,ends,match", [
    (-1, None, "lo <= hi"), (CAP + 1, None, "lo <= hi"), ((3, 2), None, "lo <= hi"), ((0, CAP + 1), None, "lo <= hi"),
    ([1] * 11, None, "holds 10"), (None, [None] * 11, "holds 10"),
    (2.0, None, "line_lengths"), (True, None, "line_lengths"), ([(1, 2, 3)], None, "line_lengths"), (["7"], None, "line_lengths"),
    ([[1], [2]], None, "rows"), (None, [[{30}], [{30}]], "rows"),
    (None, [set()], "empty"), (None, [[]], "empty"), (None, [{0, 30}], "id 0"), (None, [{30, 1}], "id 1"), (None, [{2}], "id 2"),
    (None, [{100}], "id 100"), (None, [{102}], "id 102"), (None, [{160}], "id 160"), (None, [{-3}], "id -3"),
    (None, [30], "line_end_ids"), (None, 30, "line_end_ids"), (None, [{30.5}], "line_end_ids"),
    ([0], [{30}], "hi = 0"), (0, frozenset({30}), "hi = 0"),
])
def test_check_lines_rejects(lens, ends, match):
    with pytest.raises(ValueError, match=match):
        check_lines(lens, ends, 3, 220, SENT, 160)


def test_check_lines_rejects_a_partial_prefix_line_longer_than_its_hi():
    pre = [[1] + [40] * CAP + [2, 1, 41, 42, 43]]
    with pytest.raises(ValueError, match="more than its hi = 2"):
        check_lines([None, 2], None, 1, 60, SENT, 160, prefix=pre)
    assert check_lines([None, 3], None, 1, 60, SENT, 160, prefix=pre) is not None
    with pytest.raises(ValueError, match="length >= 1"):
        check_lines(3, None, 1, 0, SENT, 160)


def test_encode_line_end():
    from mmtg_amd.generate import encode_line_end

    class Tok:
        table = {"a": 30, "b": 31, "?": 100, "p": 0, "z": 14000}

        def convert_tokens_to_ids(self, t):
            return self.table[t]

    assert encode_line_end(Tok(), "ab a\n") == frozenset({30, 31})
    for bad in ("a?", "p", "", "  ", "az"):
        with pytest.raises(ValueError):
            encode_line_end(Tok(), bad)
    assert check_lines(None, [encode_line_end(Tok(), "ab")], 1, 30, SENT, 160).sets is not None


# ------------------------------------------------------------------ ABI and validation before device work
def test_lines_entry_points_are_declared_exported_and_reject_bad_arguments_without_a_gpu():
    L = hip.lib()
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    names = ("mmtg_decode_select_lines", "mmtg_decode_sample_lines", "mmtg_decode_beam_candidates_lines")
    for name in names:
        assert "MMTG_API int %s(" % name in header
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
    for f in ("decode_select_lines", "decode_sample_lines", "decode_beam_candidates_lines"):
        assert callable(getattr(hip, f))
    p = [0x7000000000 + (i << 24) for i in range(12)]
    tail = (p[6], p[7], 10, p[8], 2, p[9], None)                              # lo, hi, n_lines, sets, n_sets, set_of, stream
    for n in (-1, SENT - 1, 1000):
        rc = L.mmtg_decode_select_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, n, *tail)
        assert rc == -1 and b"decode_select_lines: n-gram size %d outside 0..20" % n in L.mmtg_last_error()
        rc = L.mmtg_decode_sample_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[5], 8, 8, p[3], p[4], n, *tail)
        assert rc == -1 and b"decode_sample_lines: n-gram size %d outside 0..20" % n in L.mmtg_last_error()
        rc = L.mmtg_decode_beam_candidates_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[3], p[4], 8, None, n, *tail)
        assert rc == -1 and b"decode_beam_candidates_lines: n-gram size %d outside 0..20" % n in L.mmtg_last_error()
    rc = L.mmtg_decode_select_lines(None, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, 0, *tail)
    assert rc == -1 and b"decode_select_lines: the line form needs logits" in L.mmtg_last_error()
    for bad in ((None, p[7], 10, None, 0, None, None), (p[6], None, 10, None, 0, None, None), (p[6], p[7], 0, None, 0, None, None)):
        rc = L.mmtg_decode_select_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, 0, *bad)
        assert rc == -1 and b"decode_select_lines: lo / hi [B, n_lines >= 1] needed" in L.mmtg_last_error()
    for bad in ((p[6], p[7], 10, p[8], 0, p[9], None), (p[6], p[7], 10, None, 2, p[9], None), (p[6], p[7], 10, p[8], 2, None, None),
                (p[6], p[7], 10, None, -1, None, None)):
        rc = L.mmtg_decode_beam_candidates_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[3], p[4], 8, None, 3, *bad)
        assert rc == -1 and b"decode_beam_candidates_lines: end sets need sets, set_of and n_sets > 0 together" in L.mmtg_last_error()
    rc = L.mmtg_decode_select_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[2], None, 0, *tail)
    assert rc == -1 and b"decode_select_lines: pos_next must not alias pos_ptr" in L.mmtg_last_error()
    rc = L.mmtg_decode_select_lines(p[0], 40000, 40000, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], p[4], 0, *tail)
    assert rc == -1 and b"decode_select_lines: vocabulary of 40000" in L.mmtg_last_error()
    rc = L.mmtg_decode_sample_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, None, 8, 8, p[3], None, 0, *tail)
    assert rc == -1 and b"decode_sample_lines: uniforms" in L.mmtg_last_error()
    rc = L.mmtg_decode_sample_lines(p[0], 30000, 30000, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[5], 8, 8, p[3], None, 3, *tail)
    assert rc == -1 and b"decode_sample_lines: vocabulary of 30000" in L.mmtg_last_error()
    for nb in (0, 17):
        rc = L.mmtg_decode_beam_candidates_lines(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, nb, p[3], p[4], 8, p[5], 0, *tail)
        assert rc == -1 and b"decode_beam_candidates_lines: %d beams per prompt (1..16)" % nb in L.mmtg_last_error()
    rc = L.mmtg_decode_select_lines(p[0], 160, 160, p[1], 5, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, 0, *tail)
    assert rc == -1 and b"decode_select_lines: bad sequence layout" in L.mmtg_last_error()


def test_decoders_and_generate_entry_points_reject_bad_lines_before_any_device_work():
    from mmtg_amd.generate import generate_beams, generate_samples
    rows = {"topic_ids": np.zeros((1, 5), np.int64)}
    bad = (dict(line_lengths=21), dict(line_lengths=(5, 4)), dict(line_end_ids=[{1}]), dict(line_end_ids=[{160}]),
           dict(line_lengths=[0], line_end_ids=[{30}]), dict(line_lengths=[3] * 11))
    for kw in bad:
        with pytest.raises(ValueError, match="line_"):
            generate_samples(_Model(), rows, None, **kw)
        with pytest.raises(ValueError, match="line_"):
            generate_beams(_Model(), rows, None, **kw)
        for cls in (GreedyDecoder, BeamDecoder):
            dec = cls.__new__(cls)
            dec.eng = _Eng()
            dec.B, dec.max_len, dec.n_prompts, dec.nb = 1, 220, 1, 1
            with pytest.raises(ValueError, match="line_"):
                dec.begin({"img_embs": torch.zeros(1, 4)}, 220, **kw)
    dec = GreedyDecoder.__new__(GreedyDecoder)
    dec.eng = _Eng()
    dec.B, dec.max_len = 1, 220
    with pytest.raises(ValueError, match="more than its hi = 1"):
        dec.begin({"img_embs": torch.zeros(1, 4)}, 220, prefix=[[1, 40, 41]], line_lengths=[(0, 1)])


# ------------------------------------------------------------------ the CPU restatements
def cpu_lines_greedy(w, sh, table, start, length, tables, b=0, n=0, prefix=(1,), temperature=T, repetition_penalty=REP):
    """test_ngram_cpu.cpu_ngram_greedy under the line rule of tables' row b: a full line writes PAD without the logits; otherwise
    the rule's bans join the n-gram bans at -inf before the arg-max (an all -inf row picks id 0, as torch.argmax and the kernel do)."""
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
        lo, hi, ends = tables.bounds(b, c // SENT)
        x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V].clone()
        for v in banned_ids(ids, n):
            x[v] = float("-inf")
        x = apply_rule(x, ids, lo, hi, ends)
        ids.append(0 if x is None else int(torch.argmax(x).item()))
    return ids


def cpu_lines_beam_search(w, sh, table, start, length, nb, tables, b=0, n=0, prefix=(1,), temperature=T, repetition_penalty=REP):
    """test_ngram_cpu.cpu_ngram_beam_search under the line rule: a beam on a full line offers PAD with its score unchanged (what
    sticky PAD offers).  Returns (ids [nb, 1 + length] best first, scores [nb] fp32, gaps)."""
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
        lo, hi, ends = tables.bounds(b, c // SENT)
        cands = []
        for q, (cf, ids, s) in enumerate(beams):
            if s == NEG:
                cands += [(NEG, q, k, 0) for k in range(nb)]
                continue
            logits = cf(dict(base, targets=torch.tensor([ids], dtype=torch.long)))[0, -1, :]
            x = None
            if ids[-1] != 0:
                x = O.process_logits(logits, torch.tensor(ids), temperature, repetition_penalty)[:V].clone()
                for v in banned_ids(ids, n):
                    x[v] = float("-inf")
                x = apply_rule(x, ids, lo, hi, ends)
            if x is None:                                   # sticky PAD or a full line
                cands += [(s, q, 0, 0)] + [(NEG, q, k, 0) for k in range(1, nb)]
                continue
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


def end_sets_for(fx, V=160):
    """Two end sets of content ids for a fixture, taken from ids its greedy golden writes (so the model gives them some mass)."""
    seen = [v for v in dict.fromkeys(int(v) for v in fx["greedy_len220_row0"].tolist()) if v not in (0, 1, 2, 100, 102) and v < V]
    assert len(seen) >= 6
    return frozenset(seen[0:3]), frozenset(seen[3:6])


@pytest.mark.parametrize("row", [0, 1])
def test_unconstrained_tables_reproduce_the_golden_ids(row):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row%d" % row].tolist()
    for t in (check_lines([None], None, 1, 220, SENT, 160), check_lines((0, CAP), None, 1, 220, SENT, 160)):
        ids = cpu_lines_greedy(w, sh, table, start_row(batch, row), 220, t)
        assert GreedyDecoder.reference_return(ids, 220) == ref and rule_violations(ids, t, 0) == []


@pytest.mark.parametrize("row", [0, 1])
def test_seven_token_lines(row):
    """The golden lines are 20 tokens long or empty: line_lengths=7 makes every line exactly 7; line 0's seven tokens are the
    golden's first seven (later lines see another history through the repetition penalty: held to the rule only)."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row%d" % row].tolist()
    t = check_lines(7, None, 1, 220, SENT, 160)
    assert set(line_lengths_of(ref)) <= {0, 20} and rule_violations(ref, t, 0)          # the unconstrained output breaks the bounds
    ids = cpu_lines_greedy(w, sh, table, start_row(batch, row), 220, t)
    assert len(ids) == 221 and line_lengths_of(ids) == [7] * 10
    assert ids[:8] == ref[:8] and ids[8:SENT] == [0] * (SENT - 9) + [2]
    assert rule_violations(ids, t, 0) == []


def test_no_empty_lines():
    """greedy_len220_row0 has two empty lines; with lo = 1 they are not empty, and the lines before them are the golden's."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row0"].tolist()
    lens = line_lengths_of(ref)
    assert lens == [20, 20, 20, 20, 20, 20, 20, 0, 0], lens
    t = check_lines((1, CAP), None, 1, 220, SENT, 160)
    assert rule_violations(ref, t, 0)
    ids = cpu_lines_greedy(w, sh, table, start_row(batch, 0), 220, t)
    first_empty = lens.index(0)
    assert ids[:first_empty * SENT + 1] == ref[:first_empty * SENT + 1]
    got = line_lengths_of(ids)
    assert len(got) == 10 and min(got) >= 1 and got[:first_empty] == lens[:first_empty]
    assert rule_violations(ids, t, 0) == []


def test_end_sets_close_every_constrained_line_on_a_member():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    a, b_ = end_sets_for(fx)
    ends = [None, a, None, b_, None, a]
    t = check_lines([(2, 9), (2, 9), 5, (1, 6), None, (3, 3)], ends, 1, 6 * SENT, SENT, 160)
    ref = fx["greedy_len220_row1"][:6 * SENT + 1].tolist()
    assert rule_violations(ref, t, 0)
    for n in (0, 3):
        ids = cpu_lines_greedy(w, sh, table, start_row(batch, 1), 6 * SENT, t, n=n)
        assert rule_violations(ids, t, 0, n=n) == []
        got = line_lengths_of(ids)
        for l, e in enumerate(ends):
            lo, hi, _ = t.bounds(0, l)
            assert lo <= got[l] <= hi
            if e is not None:
                assert ids[l * SENT + got[l]] in e, (l, ids[l * SENT:(l + 1) * SENT])


def test_beam_restatement_obeys_the_rule_and_one_beam_is_greedy():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    a, b_ = end_sets_for(fx)
    t = check_lines([(2, 6), 4, (1, 8), 3], [None, a, b_], 1, 4 * SENT, SENT, 160)
    start = start_row(batch, 1)
    for n in (0, 2):
        ids1, s1, _ = cpu_lines_beam_search(w, sh, table, start, 4 * SENT, 1, t, n=n)
        assert ids1[0].tolist() == cpu_lines_greedy(w, sh, table, start, 4 * SENT, t, n=n)
        ids, scores, _ = cpu_lines_beam_search(w, sh, table, start, 4 * SENT, 4, t, n=n)
        assert np.isfinite(scores).all() and (np.diff(scores) <= 0).all()
        assert len({tuple(r) for r in ids.tolist()}) == 4
        for r in ids.tolist():
            assert rule_violations(r, t, 0, n=n) == [], n
    # a partial given line continues under its line's bounds
    prefix = fx["greedy_len220_row1"][:1 + SENT].tolist() + [int(v) for v in fx["greedy_len220_row1"][SENT + 1:SENT + 3]]
    ids, _, _ = cpu_lines_beam_search(w, sh, table, start, 4 * SENT, 4, t, prefix=prefix)
    for r in ids.tolist():
        assert r[:len(prefix)] == prefix and rule_violations(r, t, 0, start=len(prefix)) == []
        assert line_lengths_of(r)[1] == 4


# ------------------------------------------------------------------ which entry a step ends in
def test_every_step_ends_in_the_entry_the_dispatch_table_names(monkeypatch):
    """All sixteen (with_head, prefix, n-gram, lines) inputs, for greedy / sampled steps and for beam steps: select_forms, and the
    entries GreedyDecoder._select and BeamDecoder._select then call (recorded in place of the library, with their argument counts
    held to the ABI's), against the table written out here."""
    from types import SimpleNamespace as NS

    from mmtg_amd.decode import StepRules, select_forms
    #        with_head prefix ngram lines   select / sample / candidates   merge
    table = [(True, False, 0, False,        "",                            ""),
             (True, True, 0, False,         "_fixed",                      "_fixed"),
             (True, False, 3, False,        "_ngram",                      ""),
             (True, True, 3, False,         "_ngram",                      "_fixed"),
             (True, False, 0, True,         "_lines",                      ""),
             (True, True, 0, True,          "_lines",                      "_fixed"),
             (True, False, 3, True,         "_lines",                      ""),
             (True, True, 3, True,          "_lines",                      "_fixed"),
             (False, False, 0, False,       "",                            ""),
             (False, True, 0, False,        "_fixed",                      "_fixed"),
             (False, False, 3, False,       "",                            ""),
             (False, True, 3, False,        "_fixed",                      "_fixed"),
             (False, False, 0, True,        "",                            ""),
             (False, True, 0, True,         "_fixed",                      "_fixed"),
             (False, False, 3, True,        "",                            ""),
             (False, True, 3, True,         "_fixed",                      "_fixed")]
    assert len({r[:4] for r in table}) == 16
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
    B, nb, V = 4, 2, 160
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    lines = (torch.zeros(B, 3, dtype=torch.uint8), torch.full((B, 3), CAP, dtype=torch.uint8), None, None)
    for with_head, prefix, ngram, with_lines, want, want_merge in table:
        assert select_forms(with_head, prefix, ngram, with_lines) == (want, want_merge)
        fe = i32(B)
        logits = torch.zeros(B, V)
        dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, nb=nb, n_prompts=B // nb,
                 rules=StepRules(prefix=prefix, ngram=ngram, lines=lines if with_lines else None), copy_step=False, fixed_end=fe,
                 logits=logits, select_rows=B, select_logits=logits, seq=torch.zeros(B, 64, dtype=torch.long),
                 pos=i32(1), pos_next=i32(1), uniforms=torch.zeros(70, B), keep=i32(B, 64), rows=i32(B, 64), scores=torch.zeros(B),
                 cand_val=torch.zeros(B, nb), cand_id=i32(B, nb))
        # the graph key comes from the same answer: "prefix", then ("ngram", n), then "lines" exactly on a head step under line constraints
        dec.params = (1.1, 1.5, 1, 0.0)
        assert GreedyDecoder._graph_key(dec, with_head, 1) == (
            (with_head, 1, dec.params) + (("prefix",) if prefix else ()) + (("ngram", ngram) if ngram else ())
            + (("lines", "bounds") if with_head and with_lines else ()))
        for params, kind in (((1.1, 1.5, 1, 0.0), "select"), ((1.1, 1.5, 5, 0.9), "sample" if with_head else "select")):
            del calls[:]
            dec.params = params
            GreedyDecoder._select(dec, with_head)
            assert [c[0] for c in calls] == ["mmtg_decode_" + kind + want]
            a = calls[0][1]
            assert (a[0] != 0) == with_head                                       # logits null exactly when no head was called
            if want:                                                              # fixed_end follows pos_next: given with a prefix only
                at = 15 if kind == "sample" else 11
                assert a[at] == dec.pos_next.data_ptr() and a[at + 1] == (fe.data_ptr() if prefix else 0)
            if want in ("_ngram", "_lines"):
                assert a[at + 2] == ngram
        del calls[:]
        dec.params = (1.1, 1.5, 1, 0.0)
        BeamDecoder._select(dec, with_head)
        assert [c[0] for c in calls] == (["mmtg_decode_beam_candidates" + want] if with_head else []) + ["mmtg_decode_beam_merge" + want_merge]
        merge = calls[-1][1]
        assert (merge[0] != 0) == with_head and (merge[1] != 0) == with_head      # candidates null when no head was called
        if want_merge:
            assert merge[15] == fe.data_ptr()
        if with_head and want:
            assert calls[0][1][14] == (fe.data_ptr() if prefix else 0)
