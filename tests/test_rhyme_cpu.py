"""Rhyme schemes (rhyme_scheme= / rhyme_classes= / rhyme_distinct=) on the host: a restatement of the rule of include/mmtg_hip.h
checked on hand-written columns, check_lines' new arguments, encode_rhyme_classes, the new ABI entries' argument checks,
select_forms, and the CPU restatements of greedy decoding and beam search under the rule that tests/test_rhyme_gpu.py holds the
decoders to.

The restatements are those of tests/test_template_cpu.py, wrapped once more: while they run, the function they call for the line rule
hands a follower line the end set its leader's ending names in the row's own history -- the class of the leader line's last content
id, with rhyme_distinct minus the ids the earlier lines of the group ended on -- and leaves every other line as it is (a leader's
static end set is already in the packed tables)."""
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
from test_template_cpu import _TemplateRule, content_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the rule
def line_end(g, r, sent=SENT):
    """The last content id of line r of history g (None: the line is empty)."""
    body = [int(v) for v in g[r * sent + 1:r * sent + sent - 1] if int(v) != 0]
    return body[-1] if body else None


def rhyme_ends(g, tables, b, sent=SENT):
    """The end set the scheme gives the line a row with history g is writing (None: the line is no follower, or its leader's line is
    empty or ended on an id without a class)."""
    l = len(g) // sent
    r = tables.leader(b, l)
    if r is None:
        return None
    t = line_end(g, r, sent)
    k = None if t is None else tables.rhyme_class(t)
    if k is not None and tables.distinct:
        k = k - {line_end(g, m, sent) for m in range(l) if m == r or tables.leader(b, m) == r}
    return k


def rhyme_line_rule(g, tables, b, sent=SENT):
    """line_rule for the column after history g under row b's bounds, end sets and scheme."""
    lo, hi, ends = tables.bounds(b, len(g) // sent)
    e = rhyme_ends(g, tables, b, sent)
    assert e is None or ends is None, "a follower has no static end set"
    return line_rule(g, lo, hi, ends if e is None else e, sent)


def _line(*content):
    return [1] + list(content) + [0] * (CAP - len(content)) + [2]


K1, K2, K3 = frozenset({30, 31, 32}), frozenset({40, 41, 42}), frozenset({50, 51, 52})


def test_rule_on_hand_written_columns():
    t = check_lines([None, (0, 3), None, (0, 3)], None, 1, 4 * SENT, SENT, 160, rhyme_scheme="AABB", rhyme_classes=[K1, K2, K3])
    # leader (line 0): the static end set, the union of the classes
    assert t.bounds(0, 0) == (0, CAP, K1 | K2 | K3) and t.leader(0, 0) is None and t.leader(0, 1) == 0 and t.leader(0, 3) == 2
    assert rhyme_line_rule([1], t, 0) == (True, None)                              # a leader is never empty
    assert rhyme_line_rule([1, 77], t, 0) == (True, None) and rhyme_line_rule([1, 77, 41], t, 0) == (False, None)
    assert rhyme_line_rule([1] + [77] * (CAP - 1), t, 0) == (True, K1 | K2 | K3)   # c == hi - 1: the union
    # follower (line 1) of a leader that ended on 41: class K2
    first = _line(77, 78, 41)
    assert rhyme_ends(first + [1], t, 0) == K2
    assert rhyme_line_rule(first + [1], t, 0) == (True, None)                      # PAD banned: the previous token [#START#] is no member
    assert rhyme_line_rule(first + [1, 40], t, 0) == (False, None)                 # 40 is a member: the line may end
    assert rhyme_line_rule(first + [1, 40, 77], t, 0) == (True, K2)                # c == hi - 1 = 2: class K2 alone
    assert rhyme_line_rule(first + [1, 40, 77, 41], t, 0) == "pad"
    # the leader's own id is allowed without distinct
    assert 41 in rhyme_line_rule(first + [1, 40, 77], t, 0)[1]
    # a leader that ended earlier than hi (PAD after a member): the last non-PAD id counts
    assert rhyme_ends(_line(31) + [1], t, 0) == K1
    # class-less leader endings (an empty line, an id outside every class -- reachable through n-gram bans or a given line): no rule
    assert rhyme_ends(_line() + [1], t, 0) is None and rhyme_ends(_line(77, 78) + [1], t, 0) is None
    assert rhyme_line_rule(_line(77, 78) + [1, 90, 91], t, 0) == (False, None) and rhyme_line_rule(_line(77, 78) + [1], t, 0) == (False, None)
    # the second group finds its own leader (line 2), whatever line 0 / 1 rhymed on
    two = first + _line(40) + _line(77, 52)
    assert rhyme_ends(two + [1], t, 0) == K3 and rhyme_line_rule(two + [1, 50, 77], t, 0) == (True, K3)
    # a line after the scheme, singleton groups and '.': untouched
    t2 = check_lines(None, None, 1, 5 * SENT, SENT, 160, rhyme_scheme="ABCB", rhyme_classes=[K1, K2, K3])
    assert [t2.leader(0, l) for l in range(5)] == [None, None, None, 1, None]
    assert t2.bounds(0, 0)[2] is None and t2.bounds(0, 2)[2] is None and t2.bounds(0, 1)[2] == K1 | K2 | K3
    t3 = check_lines(None, None, 1, 4 * SENT, SENT, 160, rhyme_scheme="A.A.", rhyme_classes=[K1, K2, K3])
    assert [t3.leader(0, l) for l in range(4)] == [None, None, 0, None]
    # distinct: the ids the earlier lines of the group ended on leave the set, for the mask and for PAD
    d = check_lines((0, 3), None, 1, 3 * SENT, SENT, 160, rhyme_scheme="AAA", rhyme_classes=[K1, K2, K3], rhyme_distinct=True)
    assert d.distinct and not t.distinct
    assert rhyme_ends(first + [1], d, 0) == K2 - {41}
    assert rhyme_line_rule(first + [1, 41], d, 0) == (True, None)                  # the line cannot end on 41 again
    assert rhyme_line_rule(first + [1, 40], d, 0) == (False, None)
    assert rhyme_line_rule(first + [1, 40, 41], d, 0) == (True, K2 - {41})
    assert rhyme_ends(first + _line(40) + [1], d, 0) == K2 - {41, 40}              # the third line: both earlier endings are gone
    assert rhyme_line_rule(first + _line(77, 40) + [1, 41, 40], d, 0) == (True, frozenset({42}))


def rhyme_violations(ids, tables, b, start=1, n=0, sent=SENT):
    """test_template_cpu.template_violations with a follower's end set taken from the row's own history: the columns c >= start of
    row ids that break the line rule, the template or the scheme of tables' row b given the columns before them."""
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
        y = tables.symbol(b, c // sent, q - 1)
        r = rhyme_line_rule(ids[:c], tables, b, sent)
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


def followers_rhyme(ids, tables, b, sent=SENT):
    """[(follower line, leader line, rhymes)] for every follower of row b whose leader ended on an id with a class: rhymes says the
    follower's last content id is in that class (and, with rhyme_distinct, is none of the group's earlier endings)."""
    ids = [int(v) for v in ids]
    out = []
    for l in range(len(ids) // sent):
        e = rhyme_ends(ids[:l * sent + 1], tables, b, sent)
        if e is not None:
            out.append((l, tables.leader(b, l), line_end(ids, l, sent) in e))
    return out


def test_the_violation_checker_sees_a_broken_rhyme():
    t = check_lines(None, None, 1, 2 * SENT, SENT, 160, rhyme_scheme="AA", rhyme_classes=[K1, K2])
    good = _line(77, 41) + _line(78, 40) + [1]
    assert rhyme_violations(good, t, 0) == [] and followers_rhyme(good, t, 0) == [(1, 0, True)]
    bad = _line(77, 41) + _line(78, 30) + [1]
    assert rhyme_violations(bad, t, 0) == [SENT + 3] and followers_rhyme(bad, t, 0) == [(1, 0, False)]   # PAD after a non-member
    assert rhyme_violations(_line(77, 78) + _line(78, 30) + [1], t, 0) == [3]      # the leader ended outside every class
    d = check_lines(None, None, 1, 2 * SENT, SENT, 160, rhyme_scheme="AA", rhyme_classes=[K1, K2], rhyme_distinct=True)
    same = _line(77, 41) + _line(78, 41) + [1]
    assert rhyme_violations(same, t, 0) == [] and rhyme_violations(same, d, 0) == [SENT + 3]
    assert followers_rhyme(same, d, 0) == [(1, 0, False)]


# ------------------------------------------------------------------ check_lines(rhyme_scheme=, rhyme_classes=, rhyme_distinct=)
def test_check_lines_packs_every_accepted_scheme_form():
    cls = [K1, {40, 41, 42}, [50, 51, 52]]
    U = K1 | K2 | K3
    assert check_lines(None, None, 3, 220, SENT, 160, rhyme_scheme=None, rhyme_classes=None) is None
    t = check_lines(None, None, 3, 220, SENT, 160, rhyme_scheme="AABB", rhyme_classes=cls)                 # one string for all rows
    assert isinstance(t, LineTables) and t.lead.shape == (3, 10) and t.lead.dtype == np.int8 and t.class_of.dtype == np.int16
    assert t.lead.tolist() == [[-1, 0, -1, 2] + [-1] * 6] * 3 and t.set_of[0].tolist() == [0, -1, 0, -1] + [-1] * 6
    assert t.members(0) == U and t.tmpl is None and not t.distinct and t.class_of.shape == (160,)
    assert t.sets.shape == (4, 5)                                              # the union and the three classes, each stored once
    for k in (K1, K2, K3):
        assert {t.members(int(t.class_of[v])) for v in k} == {k}
    assert sorted(np.nonzero(t.class_of >= 0)[0].tolist()) == sorted(U) and t.rhyme_class(77) is None and t.rhyme_class(41) == K2
    assert (t.lo == 0).all() and (t.hi == CAP).all()                           # a leader's lo stays: its end set makes it non-empty
    t = check_lines(None, None, 3, 220, SENT, 160, rhyme_scheme=["ABAB", None, "a.a"], rhyme_classes=cls)   # per row, None rows
    assert t.lead[:, :4].tolist() == [[-1, -1, 0, 1], [-1] * 4, [-1, -1, 0, -1]] and t.set_of[1].tolist() == [-1] * 10
    t = check_lines(None, None, 1, 220, SENT, 160, rhyme_scheme="ABCB", rhyme_classes=cls)                 # groups of one line are free
    assert t.lead[0, :4].tolist() == [-1, -1, -1, 1] and t.set_of[0, :4].tolist() == [-1, 0, -1, -1]
    for free in ("", ".....", "ABCD", "aA"):                                   # nothing rhymes: the tables of no constraint (letters are
        t = check_lines(None, None, 2, 220, SENT, 160, rhyme_scheme=free, rhyme_classes=cls)               # symbols: a and A differ)
        assert (t.lead == -1).all() and (t.set_of == -1).all() and t.sets.shape[0] == 3
    # a leader's own end set is intersected with the union
    t = check_lines(None, [{31, 41, 77}], 1, 220, SENT, 160, rhyme_scheme="AA", rhyme_classes=cls)
    assert t.bounds(0, 0)[2] == frozenset({31, 41}) and t.leader(0, 1) == 0
    # classes shared with end sets and template classes are stored once
    t = check_lines(None, [None, None, K1], 1, 220, SENT, 160, templates=[(K2, Ellipsis)], rhyme_scheme="AA", rhyme_classes=cls)
    assert t.sets.shape[0] == 4 and t.tmpl is not None
    # templates on followers: open, or closed with a free / wide enough last column
    wide = frozenset({30, 40, 50, 77})
    t = check_lines(None, None, 1, 220, SENT, 160, templates=[None, (77, None), (78, wide)], rhyme_scheme="AAA", rhyme_classes=cls)
    assert t.hi[0, :3].tolist() == [CAP, 2, 2] and t.lead[0, :3].tolist() == [-1, 0, 0]
    assert check_lines(None, None, 1, 220, SENT, 160, templates=[None, (77, 78, Ellipsis)], rhyme_scheme="AA", rhyme_classes=cls) is not None
    assert check_lines(None, None, 1, 220, SENT, 160, templates=[(77, 41)], rhyme_scheme="AA", rhyme_classes=cls) is not None   # a leader's given end
    # distinct, and the rows carried through repeat / take
    t = check_lines(None, None, 2, 220, SENT, 160, rhyme_scheme=["AAA", "AB"], rhyme_classes=cls, rhyme_distinct=True)
    assert t.distinct
    r = t.repeat(2)
    assert r.lead.tolist() == [t.lead[0].tolist()] * 2 + [t.lead[1].tolist()] * 2 and r.distinct and r.class_of is t.class_of
    k = r.take([3, 0])
    assert k.lead.tolist() == [t.lead[1].tolist(), t.lead[0].tolist()] and k.distinct and k.class_of is t.class_of
    old = LineTables(t.lo, t.hi, None, None, SENT, 160)                        # the positional constructor
    assert old.lead is None and old.class_of is None and old.distinct is False and old.leader(0, 1) is None and old.rhyme_class(41) is None


CLS = [K1, K2, K3]


@pytest.mark.parametrize("kw,match", [
    (dict(rhyme_scheme="AA"), "rhyme_scheme and rhyme_classes come together"),
    (dict(rhyme_classes=CLS), "rhyme_scheme and rhyme_classes come together"),
    (dict(rhyme_distinct=True), "rhyme_distinct without a rhyme_scheme"),
    (dict(line_lengths=7, rhyme_distinct=True), "rhyme_distinct without a rhyme_scheme"),
    (dict(rhyme_scheme="A1", rhyme_classes=CLS), "row 0: 'A1' holds symbols other than letters"),
    (dict(rhyme_scheme="A A", rhyme_classes=CLS), "symbols other than letters"), (dict(rhyme_scheme="A-A", rhyme_classes=CLS), "symbols other"),
    (dict(rhyme_scheme=["AA", "A?", None], rhyme_classes=CLS), "row 1: 'A\\?' holds symbols"),
    (dict(rhyme_scheme=7, rhyme_classes=CLS), "rhyme_scheme: a string"), (dict(rhyme_scheme=["AA", 7, None], rhyme_classes=CLS), "rhyme_scheme: a string"),
    (dict(rhyme_scheme=["AA", "BB"], rhyme_classes=CLS), "rhyme_scheme has 2 rows, the generation 3"),
    (dict(rhyme_scheme="A" * 11, rhyme_classes=CLS), "row 0 has 11 lines, a generation of length 220 holds 10"),
    (dict(rhyme_scheme="AA", rhyme_classes=[]), "rhyme_classes: a non-empty list"), (dict(rhyme_scheme="AA", rhyme_classes={30, 31}), "rhyme_classes: a non-empty list"),
    (dict(rhyme_scheme="AA", rhyme_classes=[K1, set()]), "class 1: the class is empty"),
    (dict(rhyme_scheme="AA", rhyme_classes=[K1, 40]), "class 1: a collection of ids"), (dict(rhyme_scheme="AA", rhyme_classes=[K1, {40.5}]), "class 1: a collection of ids"),
    (dict(rhyme_scheme="AA", rhyme_classes=[K1, {32, 40}]), "id 32 is in classes 0 and 1"),
    (dict(rhyme_scheme="AA", rhyme_classes=[{0, 30}]), "class 0: id 0 "), (dict(rhyme_scheme="AA", rhyme_classes=[K1, {1}]), "class 1: id 1 "),
    (dict(rhyme_scheme="AA", rhyme_classes=[{100}]), "id 100"), (dict(rhyme_scheme="AA", rhyme_classes=[{102}]), "id 102"),
    (dict(rhyme_scheme="AA", rhyme_classes=[{160}]), "id 160"), (dict(rhyme_scheme="AA", rhyme_classes=[{-3}]), "id -3"),
    (dict(rhyme_scheme="..", rhyme_classes=[{2}]), "id 2 "),                                                # checked whatever the scheme
    (dict(line_end_ids=[None, K1], rhyme_scheme="AA", rhyme_classes=CLS), "row 0, line 1: a follower line takes no line_end_ids set"),
    (dict(line_end_ids=[{77, 78}], rhyme_scheme="AA", rhyme_classes=CLS), "row 0, line 0: no id of the line's end set has a rhyme class"),
    (dict(line_lengths=[None, 0], rhyme_scheme="AA", rhyme_classes=CLS), "row 0, line 1: a rhyming line with hi = 0"),
    (dict(line_lengths=[0], rhyme_scheme="AA", rhyme_classes=CLS), "row 0, line 0: a rhyming line with hi = 0"),
    (dict(templates=[None, (77, 41)], rhyme_scheme="AA", rhyme_classes=CLS), "row 0, line 1: a follower line of the rhyme scheme ends on the given id 41"),
    (dict(templates=[None, (77, K1 | K2)], rhyme_scheme="AA", rhyme_classes=CLS), "line 1: the last column's class leaves a rhyme class with fewer than 1 ids"),
    (dict(line_lengths=[None, 2], templates=[None, (77, K1, Ellipsis)], rhyme_scheme="AA", rhyme_classes=CLS), "leaves a rhyme class with fewer than 1"),
    (dict(templates=[(77, 78)], rhyme_scheme="AA", rhyme_classes=CLS), "row 0, line 0: the line ends on the given id 78"),   # a leader's end set
    (dict(templates=[None, None, (77, frozenset({30, 40, 50, 77}))], rhyme_scheme="AAA", rhyme_classes=CLS, rhyme_distinct=True),
     "line 2: the last column's class leaves a rhyme class with fewer than 3 ids"),
    (dict(rhyme_scheme="AAAA", rhyme_classes=CLS, rhyme_distinct=True), "rhyme_distinct and group 'A' of 4 lines, but a rhyme class of 3 ids"),
    (dict(rhyme_scheme="AABAB", rhyme_classes=[K1, {40, 41}], rhyme_distinct=True), "group 'A' of 3 lines, but a rhyme class of 2 ids"),
])
def test_check_lines_rejects_bad_schemes(kw, match):
    kw = dict(kw)
    with pytest.raises(ValueError, match=match):
        check_lines(kw.pop("line_lengths", None), kw.pop("line_end_ids", None), 3, 220, SENT, 160, **kw)


def test_schemes_the_checks_accept_beside_the_rejected_ones():
    assert check_lines(None, None, 1, 220, SENT, 160, rhyme_scheme="AAA", rhyme_classes=CLS, rhyme_distinct=True) is not None
    assert check_lines(None, None, 1, 220, SENT, 160, rhyme_scheme="AAAA", rhyme_classes=CLS) is not None            # without distinct
    assert check_lines([None, 0], None, 1, 220, SENT, 160, rhyme_scheme="A.A", rhyme_classes=CLS) is not None         # the empty line rhymes with none
    assert check_lines(None, [None, K1], 1, 220, SENT, 160, rhyme_scheme="A.A", rhyme_classes=CLS) is not None        # an end set off the scheme
    assert check_lines(None, None, 1, 220, SENT, 160, templates=[None, (77, K1 | {40, 50})], rhyme_scheme="AA", rhyme_classes=CLS) is not None
    with pytest.raises(ValueError, match="a scheme serves up to 128"):
        check_lines(None, None, 1, 129 * 3, 3, 160, rhyme_scheme="AA", rhyme_classes=CLS)


def test_encode_rhyme_classes():
    from mmtg_amd.generate import encode_line_end, encode_rhyme_classes

    class Tok:
        table = {"a": 30, "b": 31, "c": 32, "d": 40, "u": 100, "p": 0, "z": 14000, " ": 0}

        def convert_tokens_to_ids(self, t):
            return self.table[t]

    tok = Tok()
    got = encode_rhyme_classes(tok, ["ab", "c d"])
    assert got == [frozenset({30, 31}), frozenset({32, 40})] and got[0] == encode_line_end(tok, "ab")
    assert encode_rhyme_classes(tok, ["z"], vocab_cut=20000) == [frozenset({14000})]
    for bad in ([], ["ab", ""], ["ab", "bc"], ["au"], ["p"], ["az"], ["a", " "]):
        with pytest.raises(ValueError):
            encode_rhyme_classes(tok, bad)
    with pytest.raises(KeyError):
        encode_rhyme_classes(tok, ["aq"])
    t = check_lines(None, None, 1, 88, SENT, 160, rhyme_scheme="AABB", rhyme_classes=got)
    assert t.rhyme_class(40) == frozenset({32, 40})


# ------------------------------------------------------------------ ABI and validation before device work
def test_rhyme_entry_points_are_declared_exported_bound_and_reject_bad_arguments_without_a_gpu():
    lib = hip.lib()
    header = open(os.path.join(ROOT, "include", "mmtg_hip.h")).read()
    assert lib.mmtg_abi_version() == 12 and "#define MMTG_ABI_VERSION 12" in header
    for name in ("mmtg_decode_select_rhyme", "mmtg_decode_sample_rhyme", "mmtg_decode_beam_candidates_rhyme"):
        assert "MMTG_API int %s(" % name in header
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
        assert len(hip._SIGS[name][0]) == len(hip._SIGS[name.replace("_rhyme", "_tmpl")][0]) + 3
    for f in ("decode_select_rhyme", "decode_sample_rhyme", "decode_beam_candidates_rhyme"):
        assert callable(getattr(hip, f))
    p = [0x7000000000 + (i << 24) for i in range(14)]
    lines = (p[6], p[7], 10, p[8], 2, p[9])                                    # lo, hi, n_lines, sets, n_sets, set_of
    ok = (p[10], p[11], p[12], 0, None)                                        # tmpl, class_of, lead, distinct, stream
    sel = lambda lg, tail: lib.mmtg_decode_select_rhyme(lg, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, 0, *tail)      # noqa: E731
    smp = lambda lg, tail: lib.mmtg_decode_sample_rhyme(lg, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[5], 8, 8, p[3],     # noqa: E731
                                                        None, 0, *tail)
    cnd = lambda lg, tail: lib.mmtg_decode_beam_candidates_rhyme(lg, 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[3], p[4], 8,     # noqa: E731
                                                                 None, 0, *tail)
    for what, call in ((b"decode_select_rhyme", sel), (b"decode_sample_rhyme", smp), (b"decode_beam_candidates_rhyme", cnd)):
        for tail in ((p[10], None, p[12], 0, None), (None, p[11], None, 0, None)):
            assert call(p[0], lines + tail) == -1                              # a null class_of / lead (with and without templates)
            assert what + b": class_of [V] and lead [B, n_lines] are needed" in lib.mmtg_last_error()
        assert call(p[0], lines + (None, p[11], p[12], 2, None)) == -1
        assert what + b": distinct is 0 or 1 (got 2)" in lib.mmtg_last_error()
        assert call(p[0], (p[6], p[7], 10, None, 0, None) + ok) == -1          # classes are rows of sets
        assert what + b": rhyme classes are rows of sets (n_sets 0)" in lib.mmtg_last_error()
        assert call(p[0], (p[6], p[7], 129, p[8], 2, p[9]) + ok) == -1
        assert what + b": 129 lines" in lib.mmtg_last_error()
        assert call(None, lines + ok) == -1                                    # no logits
        assert what + b": the line form needs logits" in lib.mmtg_last_error()
        assert call(p[0], (None, p[7], 10, p[8], 2, p[9]) + ok) == -1          # the line tables' own checks
        assert what + b": lo / hi [B, n_lines >= 1] needed" in lib.mmtg_last_error()
    for n in (-1, SENT - 1):
        rc = lib.mmtg_decode_select_rhyme(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, n, *lines, *ok)
        assert rc == -1 and b"decode_select_rhyme: n-gram size %d outside 0..20" % n in lib.mmtg_last_error()
    rc = lib.mmtg_decode_sample_rhyme(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, None, 8, 8, p[3], None, 0, *lines, *ok)
    assert rc == -1 and b"decode_sample_rhyme: uniforms" in lib.mmtg_last_error()
    rc = lib.mmtg_decode_beam_candidates_rhyme(p[0], 160, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 17, p[3], p[4], 8, None, 0, *lines, *ok)
    assert rc == -1 and b"decode_beam_candidates_rhyme: 17 beams per prompt (1..16)" in lib.mmtg_last_error()
    # the binding's own shape checks
    tabs = (torch.zeros(8, 3, dtype=torch.uint8), torch.full((8, 3), CAP, dtype=torch.uint8), torch.zeros(2, 5, dtype=torch.int32),
            torch.zeros(8, 3, dtype=torch.int16))
    cof, lead = torch.zeros(160, dtype=torch.int16), torch.zeros(8, 3, dtype=torch.int8)
    with pytest.raises(ValueError, match="class_of must be"):
        hip._rule_tail("_rhyme", 8, 160, None, 0, tabs, None, SENT, (cof[:100], lead, False))
    with pytest.raises(ValueError, match="class_of must be"):
        hip._rule_tail("_rhyme", 8, 160, None, 0, tabs, None, SENT, (cof.int(), lead, False))
    with pytest.raises(ValueError, match="lead must be"):
        hip._rule_tail("_rhyme", 8, 160, None, 0, tabs, None, SENT, (cof, lead[:, :2].contiguous(), False))
    with pytest.raises(ValueError, match="lead must be"):
        hip._rule_tail("_rhyme", 8, 160, None, 0, tabs, None, SENT, (cof, lead.short(), False))
    with pytest.raises(ValueError, match="template table"):
        hip._rule_tail("_rhyme", 8, 160, None, 0, tabs, torch.zeros(8, 3, CAP - 1, dtype=torch.int32), SENT, (cof, lead, False))
    tail = hip._rule_tail("_rhyme", 8, 160, None, 0, tabs, None, SENT, (cof, lead, True))
    assert len(tail) == 12 and tail[-4:] == (0, cof.data_ptr(), lead.data_ptr(), 1)
    assert len(hip._rule_tail("_tmpl", 8, 160, None, 0, tabs, torch.zeros(8, 3, CAP, dtype=torch.int32), SENT)) == 9   # as before


def test_decoders_and_generate_entry_points_reject_bad_schemes_before_any_device_work():
    from mmtg_amd.generate import generate_beams, generate_samples
    rows = {"topic_ids": np.zeros((1, 5), np.int64)}
    bad = (dict(rhyme_scheme="AA"), dict(rhyme_classes=CLS), dict(rhyme_scheme="A1", rhyme_classes=CLS), dict(rhyme_scheme="A" * 11, rhyme_classes=CLS),
           dict(rhyme_scheme="AA", rhyme_classes=[K1, K1]), dict(rhyme_scheme="AA", rhyme_classes=[{13317}]),
           dict(rhyme_scheme="AA", rhyme_classes=CLS, line_end_ids=[None, {40}]), dict(rhyme_scheme="AA", rhyme_classes=CLS, line_lengths=[None, 0]),
           dict(rhyme_scheme="AA", rhyme_classes=CLS, templates=[None, (77, 41)]),
           dict(rhyme_scheme="AAAA", rhyme_classes=CLS, rhyme_distinct=True))
    for kw in bad:
        with pytest.raises(ValueError, match="rhyme|follower"):
            generate_samples(_Model(), rows, None, **kw)
        with pytest.raises(ValueError, match="rhyme|follower"):
            generate_beams(_Model(), rows, None, **kw)
        for cls in (GreedyDecoder, BeamDecoder):
            dec = cls.__new__(cls)
            dec.eng = _Eng()
            dec.B, dec.max_len, dec.n_prompts, dec.nb = 1, 220, 1, 1
            with pytest.raises(ValueError, match="rhyme|follower"):
                dec.begin({"img_embs": torch.zeros(1, 4)}, 220, **kw)
    t = check_lines(None, None, 1, 220, SENT, 13317, rhyme_scheme="AA", rhyme_classes=CLS)
    dec = GreedyDecoder.__new__(GreedyDecoder)
    dec.eng = _Eng()
    dec.B, dec.max_len = 1, 220
    with pytest.raises(ValueError, match="no line_end_ids / templates / rhyme_scheme beside them"):
        dec.begin({"img_embs": torch.zeros(1, 4)}, 220, line_lengths=t, rhyme_scheme="AA", rhyme_classes=CLS)
    with pytest.raises(ValueError, match="no line_end_ids / templates / rhyme_scheme beside them"):
        dec.begin({"img_embs": torch.zeros(1, 4)}, 220, line_lengths=t, rhyme_distinct=True)


# ------------------------------------------------------------------ which entry a step ends in
def test_select_forms_names_the_rhyme_entries_on_head_steps_only(monkeypatch):
    from types import SimpleNamespace as NS
    for with_head in (True, False):
        for prefix in (False, True):
            for ngram in (0, 3):
                for lines in (False, True):
                    for templates in (False, True):
                        was = select_forms(with_head, prefix, ngram, lines, templates=templates)
                        assert select_forms(with_head, prefix, ngram, lines, templates) == was                  # positional, as before
                        assert select_forms(with_head, prefix, ngram, lines, templates=templates, rhymes=False) == was
                        held = "_fixed" if prefix else ""
                        want = "_tmpl" if templates else "_lines" if lines else "_ngram" if ngram else held
                        assert was == ((want, held) if with_head else (held, held))
                        assert select_forms(with_head, prefix, ngram, lines, templates=templates, rhymes=True) == \
                            (("_rhyme", held) if with_head else (held, held))
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
    lines = (torch.zeros(B, 3, dtype=torch.uint8), torch.full((B, 3), CAP, dtype=torch.uint8), i32(4, 5), torch.zeros(B, 3, dtype=torch.int16))
    cof, lead = torch.zeros(V, dtype=torch.int16), torch.zeros(B, 3, dtype=torch.int8)
    for with_head in (True, False):
        for prefix in (False, True):
            for tm in (None, torch.full((B, 3, CAP), -1, dtype=torch.int32)):
                for distinct in (False, True):
                    fe = i32(B)
                    logits = torch.zeros(B, V)
                    dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, nb=nb, n_prompts=B // nb,
                             rules=StepRules(prefix=prefix, ngram=3, lines=lines, tmpl=tm, rhyme=(cof, lead, distinct)), copy_step=False,
                             fixed_end=fe, logits=logits, select_rows=B, select_logits=logits,
                             seq=torch.zeros(B, 64, dtype=torch.long), pos=i32(1), pos_next=i32(1), uniforms=torch.zeros(70, B),
                             keep=i32(B, 64), rows=i32(B, 64), scores=torch.zeros(B), cand_val=torch.zeros(B, nb), cand_id=i32(B, nb),
                             params=(1.1, 1.5, 1, 0.0))
                    held = "_fixed" if prefix else ""
                    key = GreedyDecoder._graph_key(dec, with_head, 0)
                    base = (with_head, 0, dec.params) + (("prefix",) if prefix else ()) + ("ngram", 3)
                    assert key[:len(base) + (2 if with_head else 0)] == base + (("rhyme", "sets") if with_head else ())
                    if not with_head:
                        assert key == base                                     # a step without the head: the key it always had
                    else:                                                      # what the captured launch holds by value
                        assert key[len(base) + 2:] == (("tmpl",) if tm is not None else ()) + (("distinct",) if distinct else ())
                    for params, kind in (((1.1, 1.5, 1, 0.0), "select"), ((1.1, 1.5, 5, 0.9), "sample" if with_head else "select")):
                        del calls[:]
                        dec.params = params
                        GreedyDecoder._select(dec, with_head)
                        assert [c[0] for c in calls] == ["mmtg_decode_" + kind + ("_rhyme" if with_head else held)]
                        if with_head:
                            assert calls[0][1][-5:] == (0 if tm is None else tm.data_ptr(), cof.data_ptr(), lead.data_ptr(), int(distinct), 0)
                    del calls[:]
                    dec.params = (1.1, 1.5, 1, 0.0)
                    BeamDecoder._select(dec, with_head)
                    assert [c[0] for c in calls] == (["mmtg_decode_beam_candidates_rhyme"] if with_head else []) + ["mmtg_decode_beam_merge" + held]
                    if with_head:
                        assert calls[0][1][-4:-1] == (cof.data_ptr(), lead.data_ptr(), int(distinct))
    # a record built without the argument (or with None) takes the entries and keys it always took
    logits = torch.zeros(B, V)
    dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, copy_step=False, fixed_end=i32(B), logits=logits, select_rows=B,
             select_logits=logits, seq=torch.zeros(B, 64, dtype=torch.long), pos=i32(1), pos_next=i32(1), params=(1.1, 1.5, 1, 0.0))
    for extra in ({}, {"rhyme": None}):
        dec.rules = StepRules(lines=lines[:2] + (None, None), **extra)
        del calls[:]
        GreedyDecoder._select(dec, True)
        assert [c[0] for c in calls] == ["mmtg_decode_select_lines"]
        assert GreedyDecoder._graph_key(dec, True, 0) == (True, 0, dec.params, "lines", "bounds")


# ------------------------------------------------------------------ the CPU restatements
class _RhymeRule:
    """While active, the restatements below it (test_template_cpu's wrapper, then test_lines_cpu's rule) see a follower line of row b
    with the end set rhyme_ends finds in the history."""

    def __init__(self, tables, b):
        self.tables, self.b, self.all_banned, self.followers, self.free = tables, b, 0, 0, 0

    def __call__(self, x, g, lo, hi, ends, sent=SENT):
        e = rhyme_ends(g, self.tables, self.b, sent)
        if e is not None:
            assert ends is None, "a follower has no static end set"
            self.followers += 1
            ends = e
        elif self.tables.leader(self.b, len(g) // sent) is not None:
            self.free += 1                                 # a follower whose leader gave no class
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


def cpu_rhyme_greedy(w, sh, table, start, length, tables, b=0, **kw):
    """test_template_cpu.cpu_template_greedy under row b's scheme too; returns (ids, the rhyme rule's counters)."""
    with _TemplateRule(tables, b), _RhymeRule(tables, b) as rule:
        ids = L.cpu_lines_greedy(w, sh, table, start, length, tables, b=b, **kw)
    return ids, rule


def cpu_rhyme_beam_search(w, sh, table, start, length, nb, tables, b=0, **kw):
    """test_template_cpu.cpu_template_beam_search under row b's scheme too; returns (ids, scores, gaps, the rule's counters)."""
    with _TemplateRule(tables, b), _RhymeRule(tables, b) as rule:
        ids, scores, gaps = L.cpu_lines_beam_search(w, sh, table, start, length, nb, tables, b=b, **kw)
    return ids, scores, gaps, rule


def fixture_rhymes(fx, V=160):
    """The partition the CPU and GPU tests share: four classes of ten ids each, dealt round-robin from the 40 content ids the fixture's
    golden writes first (so the model gives every class some mass), and the bounds that go with the schemes: lines of 3 .. 8 tokens
    (a 20-token golden line would end on its 20th token whatever the scheme)."""
    ids = content_ids(fx, V)
    classes = [frozenset(ids[i:40:4]) for i in range(4)]
    assert all(len(k) == 10 for k in classes) and len(frozenset().union(*classes)) == 40
    return classes, (3, 8)


@pytest.mark.parametrize("row", [0, 1])
def test_schemes_under_which_nothing_rhymes_reproduce_the_golden_ids(row):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row%d" % row].tolist()
    classes, _ = fixture_rhymes(fx)
    for scheme in (None, "..........", "ABCDEFGHIJ", "A.B"):
        t = check_lines((0, CAP), None, 1, 220, SENT, 160, rhyme_scheme=scheme, rhyme_classes=None if scheme is None else classes)
        assert (scheme is None) == (t.lead is None)
        ids, rule = cpu_rhyme_greedy(w, sh, table, start_row(batch, row), 220, t)
        assert GreedyDecoder.reference_return(ids, 220) == ref and rule.followers == 0 and rule.all_banned == 0
        assert rhyme_violations(ids, t, 0) == []


LENGTH = 5 * SENT                      # five lines: the scheme's four and one after it


@pytest.mark.parametrize("scheme", ["AABB", "ABAB"])
@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("n", [0, 3])
def test_greedy_and_beams_rhyme_under_the_scheme_and_one_beam_is_greedy(scheme, distinct, n):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    classes, bounds = fixture_rhymes(fx)
    tabs = check_lines(bounds, None, 2, LENGTH, SENT, 160, rhyme_scheme=scheme, rhyme_classes=classes, rhyme_distinct=distinct)
    for row in (0, 1):
        ids, rule = cpu_rhyme_greedy(w, sh, table, start_row(batch, row), LENGTH, tabs, b=row, n=n)
        assert rhyme_violations(ids, tabs, row, n=n) == [] and rule.followers > 0
        if n == 0:
            assert rule.all_banned == 0 and rule.free == 0                     # the host checks guarantee it
        pairs = followers_rhyme(ids, tabs, row)
        assert pairs and all(ok for _, _, ok in pairs), (row, pairs)
        if n == 0:
            assert [(l, r) for l, r, _ in pairs] == ([(1, 0), (3, 2)] if scheme == "AABB" else [(2, 0), (3, 1)])
        if distinct:
            for l, r, _ in pairs:
                assert line_end(ids, l) != line_end(ids, r)
        ids1, _, _, r1 = cpu_rhyme_beam_search(w, sh, table, start_row(batch, row), LENGTH, 1, tabs, b=row, n=n)
        assert ids1[0].tolist() == ids and r1.all_banned == rule.all_banned
    bids, scores, _, rule = cpu_rhyme_beam_search(w, sh, table, start_row(batch, 0), LENGTH, 4, tabs, b=0, n=n)
    assert np.isfinite(scores).all() and (np.diff(scores) <= 0).all() and (n > 0 or rule.all_banned == 0)
    for r in bids.tolist():                                # every beam rhymes with its own earlier lines
        assert rhyme_violations(r, tabs, 0, n=n) == [] and all(ok for _, _, ok in followers_rhyme(r, tabs, 0))


def test_the_scheme_changes_what_greedy_writes():
    """Without the follower rule (leaders alone: the union as a static end set on their lines) at least one follower ends outside its
    leader's class: the scheme is what makes the lines rhyme."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    classes, bounds = fixture_rhymes(fx)
    union = frozenset().union(*classes)
    misses = 0
    for scheme in ("AABB", "ABAB"):
        tabs = check_lines(bounds, None, 2, LENGTH, SENT, 160, rhyme_scheme=scheme, rhyme_classes=classes)
        leaders = [union if l in (tabs.leader(0, m) for m in range(4)) else None for l in range(4)]
        alone = check_lines(bounds, leaders, 2, LENGTH, SENT, 160)
        for row in (0, 1):
            ids = L.cpu_lines_greedy(w, sh, table, start_row(batch, row), LENGTH, alone, b=row)
            assert L.rule_violations(ids, alone, row) == []
            misses += sum(1 for _, _, ok in followers_rhyme(ids, tabs, row) if not ok)
    assert misses > 0
