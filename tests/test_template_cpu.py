"""Line templates (templates=) on the host: a restatement of the rule of include/mmtg_hip.h checked on hand-written columns,
check_lines(templates=), encode_template, the new ABI entries' argument checks, select_forms, and the CPU restatements of greedy
decoding and beam search under the rule that tests/test_template_gpu.py holds the decoders to.

The restatements are those of tests/test_lines_cpu.py, wrapped: while they run, the function they call for the line rule also applies
the row's template -- a given column leaves its id alone finite (at 0, so an arg-max picks it and a log_softmax offers it at
log-probability 0 with -inf fillers), a class column sets every id outside the class to -inf -- and counts the columns on which
every id ended up banned.  The runs compared with the GPU must hold none."""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_lines_cpu as L
from mmtg_amd import hip
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, StepRules, LineTables, check_lines, select_forms
from test_beam_cpu import SENT, setup_case, start_row
from test_lines_cpu import CAP, line_lengths_of, line_rule
from test_ngram_cpu import _Eng, _Model, banned_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")


# ------------------------------------------------------------------ the rule
def template_rule(g, template, lo, hi, ends, sent=SENT):
    """What the rule says of the free column a row with history g fills next, on a line whose template is `template` (the caller's
    tuple, or None), whose line_lengths bounds are lo, hi and whose end set is ends (None: no set): (forced, pad_banned, admits) --
    forced: the id the row writes without a look at the logits (a given id; PAD on a full line) or None; pad_banned and
    admits(v) (v a content id) describe the logits' column otherwise."""
    c = len(g) % sent - 1
    assert 0 <= c <= sent - 3, "a forced column"
    syms = ()
    if template is not None:
        open_ = template[-1] is Ellipsis
        syms = template[:-1] if open_ else template
        k = len(syms)
        lo, hi = (max(lo, k), hi) if open_ else (k, k)
    r = line_rule(g, lo, hi, ends, sent)
    if r == "pad":
        return 0, None, None
    y = syms[c] if c < len(syms) else None
    if isinstance(y, int):
        return y, None, None
    pad_banned, allowed = r
    return None, pad_banned, (lambda v: (allowed is None or v in allowed) and (y is None or v in y))


def test_rule_on_hand_written_columns():
    A, ends = frozenset({30, 31, 32}), frozenset({31, 40})
    t = (50, None, A, 31)                                                      # given, free, class, given: a closed line of four
    assert template_rule([1], t, 0, CAP, None)[0] == 50
    f, pad, adm = template_rule([1, 50], t, 0, CAP, None)                      # free: only PAD is banned (c < lo = 4)
    assert f is None and pad and adm(77) and adm(30)
    f, pad, adm = template_rule([1, 50, 77], t, 0, CAP, None)                  # class
    assert f is None and pad and adm(30) and not adm(77) and not adm(50)
    assert template_rule([1, 50, 77, 30], t, 0, CAP, None)[0] == 31
    assert template_rule([1, 50, 77, 30, 31], t, 0, CAP, None)[0] == 0         # closed: the line is full at k
    # the same symbols, open: the line goes on under the line rule alone (lo = 4, hi as it was)
    o = t + (Ellipsis,)
    assert template_rule([1, 50, 77, 30], o, 0, 6, None)[0] == 31
    f, pad, adm = template_rule([1, 50, 77, 30, 31], o, 0, 6, None)
    assert f is None and not pad and adm(77)
    assert template_rule([1, 50, 77, 30, 31, 60, 61], o, 0, 6, None)[0] == 0   # full at hi = 6
    f, pad, adm = template_rule([1, 50, 77, 30, 31], o, 5, 6, None)            # lo = max(5, 4): PAD still banned at c = 4
    assert f is None and pad
    # a class meeting an end set on the last column: an id needs both
    f, pad, adm = template_rule([1, 50], (50, A), 0, CAP, ends)
    assert f is None and pad and adm(31) and not adm(30) and not adm(40)
    # an open template on a line with an end set: the class column is not the last one, the set acts at hi - 1 only
    f, pad, adm = template_rule([1, 50], (50, A, Ellipsis), 0, 4, ends)
    assert adm(30) and not adm(40)
    f, pad, adm = template_rule([1, 50, 30, 60], (50, A, Ellipsis), 0, 4, ends)
    assert pad and adm(40) and adm(31) and not adm(30)                         # c = hi - 1: the end set alone; 60 is no member: PAD banned
    # a given token as the end set's predecessor: an ordinary previous token
    f, pad, adm = template_rule([1, 31], (31, Ellipsis), 0, 4, ends)
    assert f is None and not pad                                               # 31 is a member: the line may end after it
    f, pad, adm = template_rule([1, 50], (50, Ellipsis), 0, 4, ends)
    assert f is None and pad                                                   # 50 is none
    # no template, and a line after one: the line rule
    assert template_rule([1], None, 2, 4, None)[:2] == (None, True) and template_rule([1, 40, 41], None, 2, 4, None)[1] is False
    first = [1, 50] + [0] * (CAP - 1) + [2]
    assert template_rule(first + [1], (60, 61), 0, CAP, None)[0] == 60 and template_rule(first + [1, 60], (60, 61), 0, CAP, None)[0] == 61
    # the packed tables say the same
    tabs = check_lines([None, (0, 6)], [ends], 1, 2 * SENT, SENT, 160, templates=[(50, A), o])
    assert tabs.bounds(0, 0)[:2] == (2, 2) and tabs.bounds(0, 1)[:2] == (4, 6)
    assert tabs.symbol(0, 0, 0) == 50 and tabs.symbol(0, 0, 1) == A and tabs.symbol(0, 0, 2) is None
    assert [tabs.symbol(0, 1, c) for c in range(5)] == [50, None, A, 31, None] and tabs.symbol(0, 2, 0) is None


def template_violations(ids, tables, b, start=1, n=0, sent=SENT):
    """Columns c >= start of row ids that break the line rule or the template of tables' row b given the columns before them; every
    column is checked.  PAD where it is banned is no violation when the n-gram bans had emptied the column's admitted set (PAD is
    what the kernels write then), and what follows is sticky PAD."""
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
        y = tables.symbol(b, c // sent, q - 1)
        r = line_rule(ids[:c], lo, hi, ends, sent)
        if r == "pad":
            if ids[c] != 0:
                bad.append(c)
            continue
        if isinstance(y, int):
            if ids[c] != y:
                bad.append(c)
            continue
        pad_banned, allowed = r
        adm = [s for s in (allowed, y) if s is not None]
        if ids[c] == 0:
            emptied = bool(adm) and n > 0 and frozenset.intersection(*map(frozenset, adm)) <= banned_ids(ids[:c], n)
            if pad_banned and not emptied:
                bad.append(c)
        elif any(ids[c] not in s for s in adm):
            bad.append(c)
    return bad


# ------------------------------------------------------------------ check_lines(templates=)
def test_check_lines_packs_every_accepted_template_form():
    A, Bc = frozenset({30, 31}), {40, 41, 42}
    assert check_lines(None, None, 3, 220, SENT, 160, templates=None) is None
    t = check_lines(None, None, 3, 220, SENT, 160, templates=[(50, Ellipsis), None, (51, None, A)])     # one list for all rows
    assert isinstance(t, LineTables) and t.tmpl.shape == (3, 10, CAP) and t.tmpl.dtype == np.int32
    assert (t.tmpl[0] == t.tmpl[2]).all() and t.tmpl[1, 0].tolist() == [50] + [-1] * (CAP - 1) and (t.tmpl[:, 1] == -1).all()
    assert t.tmpl[0, 2].tolist() == [51, -1, -2] + [-1] * (CAP - 3) and (t.tmpl[:, 3:] == -1).all()
    assert t.lo[0].tolist() == [1, 0, 3] + [0] * 7 and t.hi[0].tolist() == [CAP, CAP, 3] + [CAP] * 7
    assert t.sets.shape == (1, 5) and t.set_of is not None and (t.set_of == -1).all() and t.members(0) == A
    t = check_lines(None, None, 3, 44, SENT, 160, templates=[[(50,)], None, [None, (Bc, Ellipsis)]])    # per row, None rows and lines
    assert t.tmpl[0, 0, 0] == 50 and (t.tmpl[1] == -1).all() and (t.tmpl[2, 0] == -1).all() and t.tmpl[2, 1, 0] == -2
    assert t.lo.tolist() == [[1, 0], [0, 0], [0, 1]] and t.hi.tolist() == [[1, CAP], [CAP, CAP], [CAP, CAP]]
    # classes and end sets share one table of distinct sets
    t = check_lines(None, [A, None, frozenset(Bc)], 2, 66, SENT, 160, templates=[(A, Bc, Ellipsis), (Bc, A), None])
    assert t.sets.shape[0] == 2 and t.set_of[0].tolist() == [0, -1, 1]
    assert t.tmpl[1, 0, :3].tolist() == [-2, -3, -1] and t.tmpl[1, 1, :3].tolist() == [-3, -2, -1]
    assert t.symbol(0, 0, 1) == frozenset(Bc) and t.symbol(0, 1, 1) == A and t.symbol(0, 5, 0) is None and t.symbol(0, 0, 99) is None
    # bounds: a closed template inside them, an open one raising lo
    t = check_lines([(2, 5), (2, 5), (4, 9)], None, 1, 66, SENT, 160, templates=[(50, 51, 52), (50, Ellipsis), (50, 51, Ellipsis)])
    assert t.lo.tolist() == [[3, 2, 4]] and t.hi.tolist() == [[3, 5, 9]]
    t = check_lines(2, None, 1, 44, SENT, 160, templates=[(50, None, Ellipsis)])                         # open with hi == k
    assert t.lo.tolist() == [[2, 2]] and t.hi.tolist() == [[2, 2]]
    t = check_lines(None, None, 1, 22, SENT, 160, templates=[tuple([None] * CAP)])
    assert t.lo.tolist() == [[CAP]] and (t.tmpl == -1).all()
    r = t.repeat(3)
    assert r.rows == 3 and r.tmpl.shape == (3, 1, CAP) and r.take([0, 2]).tmpl.shape == (2, 1, CAP)
    assert LineTables(t.lo, t.hi, None, None, SENT, 160).tmpl is None                                    # the positional constructor
    # a partial prefix line that agrees with its template
    pre = [[1] + [40] * CAP + [2, 1, 50, 30]]
    assert check_lines(None, None, 1, 60, SENT, 160, prefix=pre, templates=[None, (50, A, None, Ellipsis)]) is not None
    assert check_lines(None, None, 1, 60, SENT, 160, prefix=pre, templates=[(77,), (50, A)]) is not None   # whole given lines are not checked


A_, E_ = frozenset({30, 31}), frozenset({40, 41})


@pytest.mark.parametrize("kw,match", [
    (dict(templates=[[50], None, None]), "row 0, line 0: a tuple"), (dict(templates=[50]), "row 0, line 0: a tuple"), (dict(templates=[(50.5,)]), "row 0, line 0, column 0: an int, None or a set"),
    (dict(templates=[("a",)]), "column 0: an int, None or a set"), (dict(templates=[(50, [30, 31])]), "line 0, column 1: an int, None or a set"),
    (dict(templates=[(True,)]), "an int, None or a set"), (dict(templates=[(Ellipsis, 50)]), "column 0: an int, None or a set"),
    (dict(templates=(50,)), "templates: a list"), (dict(templates=7), "templates: a list"),
    (dict(templates=[[(50,)], (50,), None]), "row 1: a list"),
    (dict(templates=[[(50,)], None]), "templates has 2 rows"),
    (dict(templates=[()]), "row 0, line 0: 0 symbols"), (dict(templates=[(Ellipsis,)]), "line 0: 0 symbols"),
    (dict(templates=[None, tuple([50] * (CAP + 1))]), "row 0, line 1: %d symbols" % (CAP + 1)),
    (dict(templates=[(0,)]), "line 0, column 0: id 0"), (dict(templates=[(50, 1)]), "column 1: id 1 "), (dict(templates=[(2,)]), "id 2 "),
    (dict(templates=[(100,)]), "id 100"), (dict(templates=[(102,)]), "id 102"), (dict(templates=[(160,)]), "id 160"),
    (dict(templates=[(-1,)]), "id -1"), (dict(templates=[({30, 0},)]), "column 0: id 0"), (dict(templates=[(50, {30, 160})]), "column 1: id 160"),
    (dict(templates=[(50, set())]), "row 0, line 0, column 1: the class is empty"),
    (dict(line_lengths=[(1, 2)], templates=[(50, 51, 52)]), "row 0, line 0: a closed template of 3 symbols outside"),
    (dict(line_lengths=[(4, 6)], templates=[(50, 51, 52)]), "a closed template of 3 symbols outside"),
    (dict(line_lengths=[None, 2], templates=[None, (50, 51, 52, Ellipsis)]), "row 0, line 1: an open template of 3 symbols on a line with hi = 2"),
    (dict(line_end_ids=[E_], templates=[(50, 51)]), "row 0, line 0: the line ends on the given id 51"),
    (dict(line_end_ids=[E_], templates=[(50, A_)]), "row 0, line 0: the last column's class and the line's end set share no id"),
    (dict(line_lengths=[2], line_end_ids=[E_], templates=[(50, A_, Ellipsis)]), "share no id"),
    (dict(templates=[(50,)] * 11), "row 0 has 11 lines, a generation of length 220 holds 10"),
    (dict(prefix=[[1, 51]] * 3, templates=[(50, None)]), "prefix row 0 gives id 51 at column 0 of line 0, its template 50"),
    (dict(prefix=[[1, 50, 77]] * 3, templates=[(50, A_, Ellipsis)]), "prefix row 0 gives id 77 at column 1 of line 0, outside"),
    (dict(prefix=[[1, 50, 51, 52]] * 3, templates=[(50, None)]), "prefix row 0 gives 3 content tokens of line 0, more than its hi = 2"),
])
def test_check_lines_rejects_bad_templates(kw, match):
    kw = dict(kw)
    with pytest.raises(ValueError, match=match):
        check_lines(kw.pop("line_lengths", None), kw.pop("line_end_ids", None), 3, 220, SENT, 160, **kw)


def test_templates_the_checks_accept_beside_the_rejected_ones():
    assert check_lines(None, [E_], 1, 220, SENT, 160, templates=[(50, 40)]) is not None             # the given id is a member
    assert check_lines(None, [E_], 1, 220, SENT, 160, templates=[(50, {30, 41})]) is not None       # the class meets the set
    assert check_lines(None, [E_], 1, 220, SENT, 160, templates=[(50, A_, Ellipsis)]) is not None   # open: the set acts later
    t = check_lines(None, [[E_], None, [None, E_]], 3, 220, SENT, 160, templates=[(50, 40), (51, 41)])   # every row is checked
    assert t.set_of[:, :2].tolist() == [[0, -1], [-1, -1], [-1, 0]] and t.hi[:, :2].tolist() == [[2, 2]] * 3
    assert check_lines(None, None, 1, 220, SENT, 160, prefix=[[1, 50, 30]], templates=[(50, A_, 77)]) is not None


def test_encode_template():
    from mmtg_amd.generate import encode_line_end, encode_template

    class Tok:
        table = {"a": 30, "b": 31, "c": 32, "u": 100, "p": 0, "z": 14000, "?": 100, " ": 0}

        def convert_tokens_to_ids(self, t):
            return self.table[t]

    tok = Tok()
    assert encode_template(tok, "a…") == (30, Ellipsis) and encode_template(tok, "a...") == (30, Ellipsis)
    assert encode_template(tok, "a??b？c") == (30, None, None, 31, None, 32)
    level = encode_line_end(tok, "ab")
    assert encode_template(tok, "aLL?…", classes={"L": level}) == (30, level, level, None, Ellipsis)
    assert encode_template(tok, "b", classes={"b": {32}}) == (frozenset({32}),)                     # a class key wins over the character
    assert isinstance(encode_template(tok, "ab"), tuple)
    for bad in ("", "…", "...", "au", "p", "az", "a b"):
        with pytest.raises(ValueError):
            encode_template(tok, bad)
    with pytest.raises(ValueError):
        encode_template(tok, "az", vocab_cut=20000 - 6001)
    assert encode_template(tok, "z", vocab_cut=20000) == (14000,)
    t = check_lines(None, None, 2, 88, SENT, 160, templates=[encode_template(tok, ch + "…") for ch in "abca"])
    assert t.tmpl[1, :, 0].tolist() == [30, 31, 32, 30] and t.lo.tolist() == [[1] * 4] * 2


# ------------------------------------------------------------------ ABI and validation before device work
def test_template_entry_points_are_declared_exported_bound_and_reject_bad_arguments_without_a_gpu():
    lib = hip.lib()
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    assert lib.mmtg_abi_version() == 12 and "#define MMTG_ABI_VERSION 12" in header
    for name in ("mmtg_decode_select_tmpl", "mmtg_decode_sample_tmpl", "mmtg_decode_beam_candidates_tmpl"):
        assert "MMTG_API int %s(" % name in header
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
        assert len(hip._SIGS[name][0]) == len(hip._SIGS[name.replace("_tmpl", "_lines")][0]) + 1
    for f in ("decode_select_tmpl", "decode_sample_tmpl", "decode_beam_candidates_tmpl"):
        assert callable(getattr(hip, f))
    p = [0x7000000000 + (i << 24) for i in range(12)]
    lines = (p[6], p[7], 10, p[8], 2, p[9])                                    # lo, hi, n_lines, sets, n_sets, set_of
    sel = lambda lg, tail: lib.mmtg_decode_select_tmpl(lg, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, 0, *tail)      # noqa: E731
    smp = lambda lg, tail: lib.mmtg_decode_sample_tmpl(lg, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[5], 8, 8, p[3],     # noqa: E731
                                                       None, 0, *tail)
    cnd = lambda lg, tail: lib.mmtg_decode_beam_candidates_tmpl(lg, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[3], p[4], 8,     # noqa: E731
                                                                None, 0, *tail)
    for what, call in ((b"decode_select_tmpl", sel), (b"decode_sample_tmpl", smp), (b"decode_beam_candidates_tmpl", cnd)):
        assert call(p[0], lines + (None, None)) == -1                          # a null table
        assert what + b": the template table [B, n_lines, sent - 2] is needed" in lib.mmtg_last_error()
        assert call(None, lines + (p[10], None)) == -1                         # no logits
        assert what + b": the line form needs logits" in lib.mmtg_last_error()
        assert call(p[0], (None, p[7], 10, None, 0, None, p[10], None)) == -1  # the line tables' own checks
        assert what + b": lo / hi [B, n_lines >= 1] needed" in lib.mmtg_last_error()
    for n in (-1, SENT - 1):
        rc = lib.mmtg_decode_select_tmpl(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, n, *lines, p[10], None)
        assert rc == -1 and b"decode_select_tmpl: n-gram size %d outside 0..20" % n in lib.mmtg_last_error()
    rc = lib.mmtg_decode_sample_tmpl(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, None, 8, 8, p[3], None, 0, *lines, p[10], None)
    assert rc == -1 and b"decode_sample_tmpl: uniforms" in lib.mmtg_last_error()
    rc = lib.mmtg_decode_beam_candidates_tmpl(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 17, p[3], p[4], 8, None, 0, *lines, p[10], None)
    assert rc == -1 and b"decode_beam_candidates_tmpl: 17 beams per prompt (1..16)" in lib.mmtg_last_error()
    # the binding's own shape check
    tabs = (torch.zeros(8, 3, dtype=torch.uint8), torch.full((8, 3), CAP, dtype=torch.uint8), None, None)
    with pytest.raises(ValueError, match="template table"):
        hip._rule_tail("_tmpl", 8, 160, None, 0, tabs, torch.zeros(8, 3, CAP - 1, dtype=torch.int32), SENT)
    with pytest.raises(ValueError, match="template table"):
        hip._rule_tail("_tmpl", 8, 160, None, 0, tabs, torch.zeros(8, 3, CAP, dtype=torch.int64), SENT)
    assert len(hip._rule_tail("_tmpl", 8, 160, None, 0, tabs, torch.zeros(8, 3, CAP, dtype=torch.int32), SENT)) == 9


def test_decoders_and_generate_entry_points_reject_bad_templates_before_any_device_work():
    from mmtg_amd.generate import generate_beams, generate_samples
    rows = {"topic_ids": np.zeros((1, 5), np.int64)}
    bad = (dict(templates=[(1,)]), dict(templates=[(50, set())]), dict(templates=[[50]]), dict(templates=[(50,)] * 11),
           dict(templates=[(50, 51, 52)], line_lengths=[2]), dict(templates=[(50, 51)], line_end_ids=[{40}]),
           dict(templates=[(13317,)]))
    for kw in bad:
        with pytest.raises(ValueError, match="templates row 0"):
            generate_samples(_Model(), rows, None, **kw)
        with pytest.raises(ValueError, match="templates row 0"):
            generate_beams(_Model(), rows, None, **kw)
        for cls in (GreedyDecoder, BeamDecoder):
            dec = cls.__new__(cls)
            dec.eng = _Eng()
            dec.B, dec.max_len, dec.n_prompts, dec.nb = 1, 220, 1, 1
            with pytest.raises(ValueError, match="templates row 0"):
                dec.begin({"img_embs": torch.zeros(1, 4)}, 220, **kw)
    dec = GreedyDecoder.__new__(GreedyDecoder)
    dec.eng = _Eng()
    dec.B, dec.max_len = 1, 220
    with pytest.raises(ValueError, match="its template 50"):
        dec.begin({"img_embs": torch.zeros(1, 4)}, 220, prefix=[[1, 40, 41]], templates=[(50, Ellipsis)])
    with pytest.raises(ValueError, match="its template 50"):
        generate_samples(_Model(), rows, None, prefixes=[[1, 40]], templates=[[(50, Ellipsis)]])


# ------------------------------------------------------------------ which entry a step ends in
def test_select_forms_names_the_template_entries_on_head_steps_only(monkeypatch):
    from types import SimpleNamespace as NS
    today = {(True, False, 0, False): ("", ""), (True, True, 0, False): ("_fixed", "_fixed"), (True, False, 3, False): ("_ngram", ""),
             (True, True, 3, False): ("_ngram", "_fixed"), (True, False, 0, True): ("_lines", ""), (True, True, 0, True): ("_lines", "_fixed"),
             (True, False, 3, True): ("_lines", ""), (True, True, 3, True): ("_lines", "_fixed"), (False, False, 0, False): ("", ""),
             (False, True, 0, False): ("_fixed", "_fixed"), (False, False, 3, False): ("", ""), (False, True, 3, False): ("_fixed", "_fixed"),
             (False, False, 0, True): ("", ""), (False, True, 0, True): ("_fixed", "_fixed"), (False, False, 3, True): ("", ""),
             (False, True, 3, True): ("_fixed", "_fixed")}
    assert len(today) == 16
    for k, want in today.items():
        assert select_forms(*k) == want and select_forms(*k, templates=False) == want
        on = select_forms(*k, templates=True)
        assert on == (("_tmpl" if k[0] else want[0]), want[1])
        assert (on[0] == "_tmpl") == (want[0] in ("_lines", "_ngram", "_fixed", "") and k[0])
    # the entries the decoders then call, with the table as the last argument before the stream
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
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                        # noqa: E731
    lines = (torch.zeros(B, 3, dtype=torch.uint8), torch.full((B, 3), CAP, dtype=torch.uint8), None, None)
    tm = torch.full((B, 3, CAP), -1, dtype=torch.int32)
    for with_head in (True, False):
        for prefix in (False, True):
            for ngram in (0, 3):
                fe = i32(B)
                logits = torch.zeros(B, V)
                dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, nb=nb, n_prompts=B // nb,
                         rules=StepRules(prefix=prefix, ngram=ngram, lines=lines, tmpl=tm), copy_step=False, fixed_end=fe, logits=logits,
                         select_rows=B, select_logits=logits, seq=torch.zeros(B, 64, dtype=torch.long),
                         pos=i32(1), pos_next=i32(1), uniforms=torch.zeros(70, B), keep=i32(B, 64), rows=i32(B, 64),
                         scores=torch.zeros(B), cand_val=torch.zeros(B, nb), cand_id=i32(B, nb), params=(1.1, 1.5, 1, 0.0))
                held = "_fixed" if prefix else ""
                key = GreedyDecoder._graph_key(dec, with_head, 0)
                assert key == ((with_head, 0, dec.params) + (("prefix",) if prefix else ()) + (("ngram", ngram) if ngram else ())
                               + (("tmpl", "bounds") if with_head else ()))
                for params, kind in (((1.1, 1.5, 1, 0.0), "select"), ((1.1, 1.5, 5, 0.9), "sample" if with_head else "select")):
                    del calls[:]
                    dec.params = params
                    GreedyDecoder._select(dec, with_head)
                    assert [c[0] for c in calls] == ["mmtg_decode_" + kind + ("_tmpl" if with_head else held)]
                    if with_head:
                        assert calls[0][1][-2] == tm.data_ptr() and calls[0][1][-1] == 0
                del calls[:]
                dec.params = (1.1, 1.5, 1, 0.0)
                BeamDecoder._select(dec, with_head)
                assert [c[0] for c in calls] == (["mmtg_decode_beam_candidates_tmpl"] if with_head else []) + ["mmtg_decode_beam_merge" + held]
                if with_head:
                    assert calls[0][1][-2] == tm.data_ptr()


# ------------------------------------------------------------------ the CPU restatements
class _TemplateRule:
    """While active, test_lines_cpu's restatements apply row b's template of `tables` where they apply the line rule."""

    def __init__(self, tables, b):
        self.tables, self.b, self.all_banned, self.given, self.classes = tables, b, 0, 0, 0

    def __call__(self, x, g, lo, hi, ends, sent=SENT):
        j = len(g)
        y = self.tables.symbol(self.b, j // sent, j % sent - 1)
        if line_rule(g, lo, hi, ends, sent) != "pad":
            if isinstance(y, int):                     # no logits consulted: the id alone, at log-probability 0
                self.given += 1
                out = torch.full_like(x, NEG_INF)
                out[y] = 0.0
                return out
            if y is not None:
                self.classes += 1
                keep = torch.zeros_like(x, dtype=torch.bool)
                keep[sorted(y)] = True
                keep[0] = True                         # PAD stays subject to the line rule
                x = x.clone()
                x[~keep] = NEG_INF
        out = self.inner(x, g, lo, hi, ends, sent)
        if out is not None and not torch.isfinite(out).any():
            self.all_banned += 1
        return out

    def __enter__(self):
        self.inner = L.apply_rule
        L.apply_rule = self
        return self

    def __exit__(self, *exc):
        L.apply_rule = self.inner


def cpu_template_greedy(w, sh, table, start, length, tables, b=0, **kw):
    """test_lines_cpu.cpu_lines_greedy under row b's template too; returns (ids, the rule's counters)."""
    with _TemplateRule(tables, b) as rule:
        ids = L.cpu_lines_greedy(w, sh, table, start, length, tables, b=b, **kw)
    return ids, rule


def cpu_template_beam_search(w, sh, table, start, length, nb, tables, b=0, **kw):
    """test_lines_cpu.cpu_lines_beam_search under row b's template too; returns (ids, scores, gaps, the rule's counters)."""
    with _TemplateRule(tables, b) as rule:
        ids, scores, gaps = L.cpu_lines_beam_search(w, sh, table, start, length, nb, tables, b=b, **kw)
    return ids, scores, gaps, rule


def content_ids(fx, V=160):
    """Content ids of a fixture, those its greedy golden writes first (the model gives them some mass)."""
    seen = [v for v in dict.fromkeys(int(v) for r in (0, 1) for v in fx["greedy_len220_row%d" % r].tolist())
            if v not in (0, 1, 2, 100, 102) and v < V]
    rest = [v for v in range(3, V) if v not in (100, 102) and v not in seen]
    return seen + rest


def fixture_templates(fx, V=160):
    """The templates the CPU and GPU tests share, per row: an acrostic over six lines; closed lines with given ids, free columns and
    classes (of 24 and 40 ids); a mix with an end set meeting a class."""
    ids = content_ids(fx, V)
    A, Bc = frozenset(ids[0:40:2] + ids[60:64]), frozenset(ids[1:41:2] + ids[64:84])
    ends = frozenset(ids[1:9])
    acro = [(v, Ellipsis) for v in ids[10:16]]
    closed = [(ids[3], None, A, None, ids[5]), (A, Bc, A, Bc), (None, None, ids[7]), (Bc, Ellipsis), None, (ids[2], A, Bc, None, None, A, Bc)]
    mix = [(A, None, Ellipsis), (ids[4], None, None, Bc), None, (Bc, A, Ellipsis), (None,), (A, Ellipsis)]
    assert len(A) == 24 and len(Bc) == 40 and ends & Bc
    return dict(templates=[acro, closed, mix], line_lengths=[None, None, [(0, 9), None, (2, 6), (0, 4), None, (3, 8)]],
                line_end_ids=[None, None, [None, ends, None, None, None, ends]]), A, Bc, ends


@pytest.mark.parametrize("row", [0, 1])
def test_free_symbols_and_open_ends_reproduce_the_golden_ids(row):
    """The golden lines are 20 tokens long or empty: an open template of free symbols only asks for k tokens, which a 20-token line
    holds, and a template-less line is untouched."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row%d" % row].tolist()
    lens = line_lengths_of(ref)
    tm = [(None,) * min(3 + l, n) + (Ellipsis,) if n else None for l, n in enumerate(lens)]
    t = check_lines(None, None, 1, 220, SENT, 160, templates=tm)
    assert t.tmpl is not None and (t.tmpl == -1).all() and t.lo.max() > 0
    ids, rule = cpu_template_greedy(w, sh, table, start_row(batch, row), 220, t)
    assert GreedyDecoder.reference_return(ids, 220) == ref and template_violations(ids, t, 0) == [] and rule.all_banned == 0


def test_an_acrostic_opens_every_line_with_its_character():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    kw, _, _, _ = fixture_templates(fx)
    acro = kw["templates"][0]
    t = check_lines(None, None, 1, 6 * SENT, SENT, 160, templates=acro)
    for n in (0, 3):
        ids, rule = cpu_template_greedy(w, sh, table, start_row(batch, 0), 6 * SENT, t, n=n)
        assert [ids[l * SENT + 1] for l in range(6)] == [s[0] for s in acro]
        assert rule.given == 6 and rule.all_banned == 0 and template_violations(ids, t, 0, n=n) == []
        assert min(line_lengths_of(ids)) >= 1
    bids, scores, _, rule = cpu_template_beam_search(w, sh, table, start_row(batch, 0), 6 * SENT, 4, t)
    assert rule.all_banned == 0 and np.isfinite(scores).all() and (np.diff(scores) <= 0).all()
    assert len({tuple(r) for r in bids.tolist()}) == 4
    for r in bids.tolist():
        assert [r[l * SENT + 1] for l in range(6)] == [s[0] for s in acro] and template_violations(r, t, 0) == []


def test_closed_templates_fix_length_given_ids_and_classes_and_one_beam_is_greedy():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    kw, A, Bc, ends = fixture_templates(fx)
    length = 6 * SENT
    tabs = check_lines(kw["line_lengths"], kw["line_end_ids"], 3, length, SENT, 160, templates=kw["templates"])
    for row in (1, 2):
        for n in (0, 3):
            ids, rule = cpu_template_greedy(w, sh, table, start_row(batch, row), length, tabs, b=row, n=n)
            assert rule.all_banned == 0 and rule.given > 0 and rule.classes > 0
            assert template_violations(ids, tabs, row, n=n) == []
            got = line_lengths_of(ids)
            for l, e in enumerate(kw["templates"][row]):
                if e is None:
                    continue
                syms = e[:-1] if e[-1] is Ellipsis else e
                assert (got[l] >= len(syms)) if e[-1] is Ellipsis else (got[l] == len(syms)), (row, l)
                for c, y in enumerate(syms):
                    v = ids[l * SENT + 1 + c]
                    assert y is None or (v == y if isinstance(y, int) else v in y), (row, l, c)
            ids1, s1, _, r1 = cpu_template_beam_search(w, sh, table, start_row(batch, row), length, 1, tabs, b=row, n=n)
            assert ids1[0].tolist() == ids and r1.all_banned == 0
    got = line_lengths_of(cpu_template_greedy(w, sh, table, start_row(batch, 2), length, tabs, b=2)[0])
    ids = cpu_template_greedy(w, sh, table, start_row(batch, 2), length, tabs, b=2)[0]
    assert ids[SENT + 4] in ends & Bc and ids[5 * SENT + got[5]] in ends                   # the class meets the end set; an open line ends on a member
    bids, scores, _, rule = cpu_template_beam_search(w, sh, table, start_row(batch, 1), length, 4, tabs, b=1, n=2)
    assert rule.all_banned == 0 and np.isfinite(scores).all()
    for r in bids.tolist():
        assert template_violations(r, tabs, 1, n=2) == []
    # the unconstrained golden breaks the templates it would then get
    assert template_violations(fx["greedy_len220_row1"][:length + 1].tolist(), tabs, 1)
