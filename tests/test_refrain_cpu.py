"""Refrain schemes (refrain_scheme=) on the host: check_refrain and what carries its table (LineTables.src through repeat / take,
Constraints), every ValueError the argument can raise before device work, the new ABI entries' argument checks, select_forms and
the graph keys, and the CPU restatement of greedy decoding under the rule that tests/test_refrain_gpu.py holds the decoders to.

The restatement is test_rhyme_cpu.cpu_rhyme_greedy (bounds, end sets, templates, rhymes, n-gram bans: every other rule as it is
restated there) run up to each copy line, the copy written column by column from the row's own ids, and resumed behind it with the
ids so far as its prefix -- so the copied ids are ordinary history for everything after them."""
import ctypes

import numpy as np
import pytest
import torch

import test_lines_cpu as L
from mmtg_amd import hip
from mmtg_amd.constraints import _check_constraints, check_refrain
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, StepRules, LineTables, check_lines, select_forms
from test_beam_cpu import SENT, comparable_length, setup_case, start_row
from test_lines_cpu import CAP
from test_ngram_cpu import _Eng, _Model, banned_ids
from test_rhyme_cpu import LENGTH, cpu_rhyme_greedy

K1, K2 = frozenset({30, 31, 32}), frozenset({40, 41, 42})


def _line(*content):
    return [1] + list(content) + [0] * (CAP - len(content)) + [2]


# ------------------------------------------------------------------ check_refrain
def test_check_refrain_resolves_every_accepted_scheme_form():
    assert check_refrain(None, 3, 220) is None
    s = check_refrain("AAA", 2, 220)                                           # chains: every copy names the letter's FIRST line
    assert s.dtype == np.int8 and s.shape == (2, 10) and s.tolist() == [[-1, 0, 0] + [-1] * 7] * 2
    assert check_refrain("AB.A", 1, 220)[0, :5].tolist() == [-1, -1, -1, 0, -1]
    assert check_refrain("AB.AB.AB.A", 1, 220)[0].tolist() == [-1, -1, -1, 0, 1, -1, 0, 1, -1, 0]
    for free in ("", "....", "ABCDEFGHIJ", "aA", "A.b"):                       # nothing repeats ('.', letters used once; a and A differ)
        assert (check_refrain(free, 2, 220) == -1).all()
    s = check_refrain(["ABA", None, ".xx"], 3, 220)                            # per prompt, None rows
    assert s[:, :3].tolist() == [[-1, -1, 0], [-1, -1, -1], [-1, -1, 1]]
    assert (s < np.arange(10)[None, :]).all()                                  # a source lies before its copy
    assert check_refrain("AA", 1, 2 * SENT).shape == (1, 2) and check_refrain("AA", 1, SENT + 1).shape == (1, 2)
    # beside line tables: the source's bounds or the default on a copy line; a source line is an ordinary line
    t = check_lines([(2, 5), None, (2, 5)], [K1], 1, 220, SENT, 160, templates=[(77, Ellipsis)])
    assert check_refrain("A.A", 1, 220, lines=t)[0, :3].tolist() == [-1, -1, 0]
    # a whole given copy line that equals its given source, and whole given lines before the copy
    same = _line(50, 51) + _line(60) + _line(50, 51) + [1]
    assert check_refrain("A.A", 1, 220, prefix=[same])[0, 2] == 0
    assert check_refrain("A.A", 1, 220, prefix=[_line(50, 51) + _line(60) + [1]])[0, 2] == 0
    assert check_refrain("A.A", 1, 220, prefix=[_line(50, 51) + [1, 60]])[0, 2] == 0      # a partial line that is no copy line


def test_src_travels_with_the_tables_through_repeat_and_take():
    sh = _Eng().sh
    cons = _check_constraints(None, 3, None, None, 2, 220, sh, "2 rows", refrain_scheme=["AB.A", "AA"])
    t = cons.lines
    assert isinstance(t, LineTables) and t.bare and t.src.tolist() == [[-1, -1, -1, 0] + [-1] * 6, [-1, 0] + [-1] * 8]
    assert (t.lo == 0).all() and (t.hi == CAP).all() and t.sets is None and t.tmpl is None and t.lead is None
    assert t.source(0, 3) == 0 and t.source(0, 0) is None and t.source(1, 1) == 0 and t.source(1, 40) is None
    r = cons.repeat(2).lines
    assert r.src.tolist() == [t.src[0].tolist()] * 2 + [t.src[1].tolist()] * 2 and r.bare
    k = cons.repeat(2).take([3, 0]).lines
    assert k.src.tolist() == [t.src[1].tolist(), t.src[0].tolist()] and k.bare
    both = _check_constraints(None, 0, (2, 9), None, 2, 220, sh, "2 rows", refrain_scheme="AA").lines
    assert not both.bare and both.src[:, :2].tolist() == [[-1, 0]] * 2 and both.repeat(3).src.shape == (6, 10)
    assert _check_constraints(None, 0, (2, 9), None, 2, 220, sh, "2 rows").lines.src is None
    assert _check_constraints(None, 0, None, None, 2, 220, sh, "2 rows").lines is None
    old = LineTables(t.lo, t.hi, None, None, SENT, 160)                        # the positional constructor
    assert old.src is None and not old.bare and old.source(0, 3) is None
    # tables taken as checked carry their src; a scheme beside them is refused
    assert _check_constraints(None, 0, both, None, 2, 220, sh, "2 rows").lines is both
    with pytest.raises(ValueError, match="nor a refrain_scheme"):
        _check_constraints(None, 0, both, None, 2, 220, sh, "2 rows", refrain_scheme="AA")


CLS = [K1, K2]


@pytest.mark.parametrize("kw,match", [
    (dict(refrain_scheme="A1"), "row 0: 'A1' holds symbols other than letters"),
    (dict(refrain_scheme="A A"), "symbols other than letters"),
    (dict(refrain_scheme=["AA", "A?", None]), "row 1: 'A\\?' holds symbols"),
    (dict(refrain_scheme=7), "refrain_scheme: a string"), (dict(refrain_scheme=["AA", 7, None]), "refrain_scheme: a string"),
    (dict(refrain_scheme=["AA", "BB"]), "refrain_scheme has 2 rows, the generation 3"),
    (dict(refrain_scheme="A" * 11), "row 0 has 11 lines, a generation of length 220 holds 10"),
    (dict(refrain_scheme="AA", line_lengths=[(2, 5), (3, 5)]), "line 1: a copy line .* not the model's to shape.*bounds other than its source's"),
    (dict(refrain_scheme="AA", line_lengths=[None, 7]), "bounds other than its source's"),
    (dict(refrain_scheme="A.A", line_end_ids=[None, None, K1]), "line 2: a copy line .* not the model's to shape.*end set"),
    (dict(refrain_scheme="AA", templates=[None, (77, Ellipsis)]), "line 1: a copy line .* not the model's to shape.*template"),
    (dict(refrain_scheme="AA", templates=[None, (None, None)]), "not the model's to shape"),
    (dict(refrain_scheme="ABA", rhyme_scheme="XYY", rhyme_classes=CLS), "line 2: a copy line .* not the model's to shape.*rhyme letter"),
    (dict(refrain_scheme="ABA", rhyme_scheme="X.X", rhyme_classes=CLS), "not the model's to shape.*rhyme letter"),
    (dict(refrain_scheme="ABA", rhyme_scheme="XYZ", rhyme_classes=CLS), "not the model's to shape.*rhyme letter other than '.'"),
    (dict(refrain_scheme=".AA", rhyme_scheme="X.XX", rhyme_classes=CLS), "line 2: a copy line"),
    (dict(refrain_scheme="AA", prefix=[_line(50, 51) + [1, 50]] * 3), "prefix row 0 ends inside line 1, a copy line"),
    (dict(refrain_scheme="A.A", prefix=[_line(50, 51) + _line(60) + _line(50, 52) + [1]] * 3), "prefix row 0 gives line 2, a copy line .* other than its"),
    (dict(refrain_scheme="AA", prefix=[_line(50, 51) + _line(50) + [1]] * 3), "gives line 1, a copy line"),
])
def test_check_refrain_rejects(kw, match):
    sh = _Eng().sh
    kw = dict(kw)
    scheme, prefix = kw.pop("refrain_scheme"), kw.pop("prefix", None)
    with pytest.raises(ValueError, match=match):
        _check_constraints(prefix, 0, kw.pop("line_lengths", None), kw.pop("line_end_ids", None), 3, 220, sh, "3 rows",
                           kw.pop("templates", None), kw.pop("rhyme_scheme", None), kw.pop("rhyme_classes", None), False, scheme)


def test_what_a_scheme_accepts_beside_the_other_rules():
    sh = _Eng().sh
    ok = (dict(line_lengths=[(2, 5), (2, 5)]), dict(line_lengths=[(2, 5)]), dict(line_lengths=[7, None]),       # the source's, or none
          dict(line_end_ids=[K1]), dict(templates=[(77, None, Ellipsis)]),                                      # on the source line
          dict(rhyme_scheme="X.X", rhyme_classes=CLS), dict(rhyme_scheme="..XX", rhyme_classes=CLS))              # off the copy line
    for kw in ok:
        c = _check_constraints(None, 0, kw.get("line_lengths"), kw.get("line_end_ids"), 2, 220, sh, "2 rows", kw.get("templates"),
                               kw.get("rhyme_scheme"), kw.get("rhyme_classes"), False, "AA")
        assert c.lines.src[:, :3].tolist() == [[-1, 0, -1]] * 2 and not c.lines.bare
    with pytest.raises(ValueError, match="a scheme serves up to 128"):
        check_refrain("AA", 1, 129 * SENT)


def test_decoders_and_generate_entry_points_reject_bad_schemes_and_keywords_before_any_device_work():
    from mmtg_amd.generate import generate_beams, generate_samples
    rows = {"topic_ids": np.zeros((1, 5), np.int64)}
    bad = (dict(refrain_scheme="A1"), dict(refrain_scheme="A" * 11), dict(refrain_scheme="AA", line_lengths=[None, 7]),
           dict(refrain_scheme="AA", templates=[None, (77, Ellipsis)]), dict(refrain_scheme="AA", line_end_ids=[None, {40}]),
           dict(refrain_scheme="AA", rhyme_scheme=".XX", rhyme_classes=CLS))
    for kw in bad:
        with pytest.raises(ValueError, match="refrain_scheme"):
            generate_samples(_Model(), rows, None, **kw)
        with pytest.raises(ValueError, match="refrain_scheme"):
            generate_beams(_Model(), rows, None, **kw)
        for cls in (GreedyDecoder, BeamDecoder):
            dec = cls.__new__(cls)
            dec.eng = _Eng()
            dec.B, dec.max_len, dec.n_prompts, dec.nb = 1, 220, 1, 1
            with pytest.raises(ValueError, match="refrain_scheme"):
                dec.begin({"img_embs": torch.zeros(1, 4)}, 220, **kw)
    # keywords together with a scheme: the one combination left out
    with pytest.raises(ValueError, match="keywords= and refrain_scheme= are not combined"):
        generate_beams(_Model(), rows, None, refrain_scheme="AA", keywords=[[40, 41]])
    dec = BeamDecoder.__new__(BeamDecoder)
    dec.eng = _Eng()
    dec.B, dec.max_len, dec.n_prompts, dec.nb = 4, 220, 1, 4
    with pytest.raises(ValueError, match="keywords= and refrain_scheme= are not combined"):
        dec.begin({"img_embs": torch.zeros(1, 4)}, 220, refrain_scheme="AA", keywords=[[40, 41]])
    t = _check_constraints(None, 0, None, None, 1, 220, _Eng().sh, "1 row", refrain_scheme="AA").lines
    with pytest.raises(ValueError, match="keywords= and refrain_scheme= are not combined"):
        dec.begin({"img_embs": torch.zeros(1, 4)}, 220, line_lengths=t, keywords=[[40, 41]])
    with pytest.raises(ValueError, match="keywords= needs beams"):
        generate_samples(_Model(), rows, None, refrain_scheme="AA", keywords=[[40, 41]])


# ------------------------------------------------------------------ the ABI entries
def test_refrain_entry_points_are_declared_exported_and_reject_bad_arguments_without_a_gpu():
    lib = hip.lib()
    names = ("mmtg_decode_select_refrain", "mmtg_decode_sample_refrain", "mmtg_decode_beam_candidates_refrain")
    for name in names:
        assert name in hip.exported_symbols() and hasattr(ctypes.CDLL(hip.lib_path()), name)
        assert len(hip._SIGS[name][0]) == len(hip._SIGS[name.replace("_refrain", "_rhyme")][0]) + 1
    p = [0x7000000000 + (i << 24) for i in range(16)]
    full = (p[5], p[6], 3, p[7], 4, p[8], p[9], p[10], p[11], 0)               # lo, hi, n_lines, sets, n_sets, set_of, tmpl, class_of, lead, distinct
    none = (None, None, 3, None, 0, None, None, None, None, 0)                 # the "no rule" forms: n_lines is the width of src

    def select(logits, rule, src, ngram=0):
        return lib.mmtg_decode_select_refrain(logits, 168, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 8, p[3], None, ngram, *rule, src, None)

    def sample(logits, rule, src):
        return lib.mmtg_decode_sample_refrain(logits, 168, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 10, 0.7, p[4], 8, 8, p[3], None, 0, *rule, src,
                                              None)

    def cands(logits, rule, src):
        return lib.mmtg_decode_beam_candidates_refrain(logits, 168, 160, p[1], 64, p[2], 5, SENT, 1.1, 1.5, 4, p[12], p[13], 8, None, 0, *rule,
                                                       src, None)
    for rule in (full, none):                                                  # a null src fails with an error code and no launch
        for call, what in ((select, "decode_select_refrain"), (sample, "decode_sample_refrain"), (cands, "decode_beam_candidates_refrain")):
            assert call(p[0], rule, None) == -1 and (what + ": src [B, n_lines] is needed").encode() in lib.mmtg_last_error()
    assert select(None, none, None) == -1 and b"src [B, n_lines] is needed" in lib.mmtg_last_error()
    for n_lines in (0, 129, -1):                                               # n_lines outside what the rhyme entries accept
        rule = full[:2] + (n_lines,) + full[3:]
        assert select(p[0], rule, p[14]) == -1 and b"decode_select_refrain: %d lines" % n_lines in lib.mmtg_last_error()
        assert cands(p[0], rule, p[14]) == -1 and b"decode_beam_candidates_refrain: %d lines" % n_lines in lib.mmtg_last_error()
    assert select(p[0], full, p[14], ngram=21) == -1 and b"n-gram size 21 outside 0..20" in lib.mmtg_last_error()
    assert select(p[0], (p[5], None) + full[2:], p[14]) == -1 and b"lo and hi come together" in lib.mmtg_last_error()
    assert select(p[0], (None, None, 3, None, 0, None, p[9], None, None, 0), p[14]) == -1 and b"line tables without lo / hi" in lib.mmtg_last_error()
    assert select(p[0], full[:7] + (p[10], None, 0), p[14]) == -1 and b"class_of [V] and lead [B, n_lines] come together" in lib.mmtg_last_error()
    assert select(p[0], full[:7] + (None, None, 1), p[14]) == -1 and b"distinct is 0 or, with a rhyme scheme, 1" in lib.mmtg_last_error()
    assert select(p[0], full[:9] + (2,), p[14]) == -1 and b"distinct" in lib.mmtg_last_error()
    assert select(p[0], full[:3] + (None, 0, None) + full[6:], p[14]) == -1 and b"rhyme classes are rows of sets" in lib.mmtg_last_error()
    assert sample(None, full, p[14]) == -1 and b"decode_sample_refrain: a draw needs logits" in lib.mmtg_last_error()
    assert cands(None, full, p[14]) == -1 and b"decode_beam_candidates_refrain: bad args" in lib.mmtg_last_error()
    # the binding: shapes and dtypes of src, and the tail it builds
    tabs = (torch.zeros(8, 3, dtype=torch.uint8), torch.zeros(8, 3, dtype=torch.uint8), None, None)
    src = torch.full((8, 3), -1, dtype=torch.int8)
    for wrong in (src[:4], src.short(), src[:, :2].contiguous(), src.t().contiguous().t()):
        with pytest.raises(ValueError, match="src must be contiguous int8"):
            hip._rule_tail("_refrain", 8, 160, None, 0, tabs, None, SENT, None, wrong)
    tail = hip._rule_tail("_refrain", 8, 160, None, 2, tabs, None, SENT, None, src)
    assert len(tail) == 13 and tail[:2] == (0, 2) and tail[4] == 3 and tail[-5:] == (0, 0, 0, 0, src.data_ptr())
    bare = hip._rule_tail("_refrain", 8, 160, None, 0, None, None, SENT, None, src)
    assert bare == (0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, src.data_ptr())
    with pytest.raises(ValueError, match="come with line tables"):
        hip._rule_tail("_refrain", 8, 160, None, 0, None, torch.zeros(8, 3, CAP, dtype=torch.int32), SENT, None, src)
    assert len(hip._rule_tail("_rhyme", 8, 160, None, 0, tabs, None, SENT, None)) == 12                   # as before


# ------------------------------------------------------------------ which entry a step ends in
def test_select_forms_names_the_refrain_entries_exactly_when_a_scheme_is_given(monkeypatch):
    from types import SimpleNamespace as NS
    for with_head in (True, False):
        for prefix in (False, True):
            for ngram in (0, 3):
                for lines in (False, True):
                    for templates in (False, True):
                        for rhymes in (False, True):
                            for groups in (False, True):
                                a = (with_head, prefix, ngram, lines)
                                kw = dict(templates=templates, rhymes=rhymes, groups=groups)
                                was = select_forms(*a, **kw)
                                held = "_fixed" if prefix else ""
                                assert select_forms(*a, refrain=False, **kw) == was == select_forms(*a, refrain=False, copies=True, **kw)
                                got = select_forms(*a, refrain=True, **kw)
                                assert got == (("_refrain", was[1]) if with_head else (held, held))          # ahead of "_rhyme"; the merge stays
                                assert select_forms(*a, refrain=True, copies=True, **kw) == (got if with_head else ("_refrain", held))
    assert select_forms(True, False, 0, False, keywords=True) == ("_kw", "_kw")
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
    src = torch.full((B, 3), -1, dtype=torch.int8)
    for with_head, copies in ((True, False), (False, False), (False, True)):
        for prefix in (False, True):
            for ln, tm, rh in ((None, None, None), (lines, None, None), (lines[:2] + (None, None), None, None),
                               (lines, torch.full((B, 3, CAP), -1, dtype=torch.int32), None), (lines, None, (cof, lead, True)),
                               (lines, None, (cof, lead, False))):
                fe = i32(B)
                logits = torch.zeros(B, V)
                dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, nb=nb, n_prompts=B // nb,
                         rules=StepRules(prefix=prefix, ngram=3, lines=ln, tmpl=tm, rhyme=rh, refrain=src), copy_step=copies, fixed_end=fe,
                         logits=logits, select_rows=B, select_logits=logits,
                         seq=torch.zeros(B, 64, dtype=torch.long), pos=i32(1), pos_next=i32(1), uniforms=torch.zeros(70, B),
                         keep=i32(B, 64), rows=i32(B, 64), scores=torch.zeros(B), cand_val=torch.zeros(B, nb), cand_id=i32(B, nb),
                         params=(1.1, 1.5, 1, 0.0))
                held = "_fixed" if prefix else ""
                key = GreedyDecoder._graph_key(dec, with_head, 0)
                base = (with_head, 0, dec.params) + (("prefix",) if prefix else ()) + ("ngram", 3)
                if not with_head and not copies:
                    assert key == base                                         # a forced step: the key and the entry it always had
                else:                                                          # what the captured launch holds by value
                    assert key == base + ("refrain",) + (() if ln is None else ("sets" if ln[2] is not None else "bounds",)) + (
                        ("tmpl",) if tm is not None else ()) + (() if rh is None else ("rhyme",) + (("distinct",) if rh[2] else ()))
                for params, kind in (((1.1, 1.5, 1, 0.0), "select"), ((1.1, 1.5, 5, 0.9), "sample" if with_head else "select")):
                    del calls[:]
                    dec.params = params
                    GreedyDecoder._select(dec, with_head)
                    assert [c[0] for c in calls] == ["mmtg_decode_" + kind + ("_refrain" if with_head or copies else held)]
                    if with_head or copies:
                        a = calls[0][1]
                        assert a[-2:] == (src.data_ptr(), 0) and a[0] == (dec.logits.data_ptr() if with_head else 0)
                        assert a[-6:-2] == (0 if tm is None else tm.data_ptr(), 0 if rh is None else cof.data_ptr(),
                                            0 if rh is None else lead.data_ptr(), int(bool(rh and rh[2])))
                        assert a[-12:-6] == ((0, 0, 3, 0, 0, 0) if ln is None else
                                             (ln[0].data_ptr(), ln[1].data_ptr(), 3, 0 if ln[2] is None else ln[2].data_ptr(),
                                              0 if ln[2] is None else 4, 0 if ln[3] is None else ln[3].data_ptr()))
                if copies:
                    continue                                                   # (beams skip no head)
                del calls[:]
                dec.params = (1.1, 1.5, 1, 0.0)
                BeamDecoder._select(dec, with_head)
                assert [c[0] for c in calls] == (["mmtg_decode_beam_candidates_refrain"] if with_head else []) + ["mmtg_decode_beam_merge" + held]
                if with_head:
                    assert calls[0][1][-2:] == (src.data_ptr(), 0)
    # a record built without the argument (or with None) takes the entries and keys it always took, on a copy step too
    logits = torch.zeros(B, V)
    dec = NS(eng=NS(sh=NS(P=5, msl=SENT - 2, V=V), layout=NS(Vpad=V)), B=B, fixed_end=i32(B), logits=logits, select_rows=B, select_logits=logits,
             seq=torch.zeros(B, 64, dtype=torch.long), pos=i32(1), pos_next=i32(1), params=(1.1, 1.5, 1, 0.0))
    for extra, copies in (({}, False), ({"refrain": None}, False), ({"refrain": None}, True)):
        dec.rules, dec.copy_step = StepRules(lines=lines, rhyme=(cof, lead, False), **extra), copies
        for with_head in (True, False):
            del calls[:]
            GreedyDecoder._select(dec, with_head)
            assert [c[0] for c in calls] == ["mmtg_decode_select" + ("_rhyme" if with_head else "")]
        assert GreedyDecoder._graph_key(dec, True, 0) == (True, 0, dec.params, "rhyme", "sets")
        assert GreedyDecoder._graph_key(dec, False, 0) == (False, 0, dec.params)


def test_which_columns_skip_the_head(monkeypatch):
    """GreedyDecoder._copy_columns: a column skips the head when every row is held by its prefix or copies there and one at least
    copies; never with return_logprobs, never for beams, never with the switch off."""
    from types import SimpleNamespace as NS
    sh = _Eng().sh
    dec = NS(eng=NS(sh=NS(msl=SENT - 2)), _skips_copies=True)
    cols = lambda *a, **k: GreedyDecoder._copy_columns(dec, *a, **k)           # noqa: E731
    t = _check_constraints(None, 0, None, None, 2, 4 * SENT, sh, "2 rows", refrain_scheme="AB.A").lines
    want = np.zeros(1 + 4 * SENT, bool)
    want[3 * SENT + 1:3 * SENT + 1 + CAP] = True
    assert cols(t, None, 4 * SENT, False).tolist() == want.tolist()
    assert cols(t, None, 4 * SENT, True) is None                               # return_logprobs wants the head's word on every column
    mixed = _check_constraints(None, 0, None, None, 2, 4 * SENT, sh, "2 rows", refrain_scheme=["AB.A", "ABAB"]).lines
    assert cols(mixed, None, 4 * SENT, False).tolist() == want.tolist()        # line 2: row 0 chooses, so the head runs
    assert cols(_check_constraints(None, 0, None, None, 2, 4 * SENT, sh, "2 rows", refrain_scheme=["AA", None]).lines, None, 4 * SENT,
                False) is None
    # a row held by its prefix where the other copies: skipped; where every row is held: the prefix shortcut's, not this one's
    pre = [_line(50, 51) + _line(50, 51) + [1, 52], [1]]
    got = cols(_check_constraints(pre, 0, None, None, 2, 4 * SENT, sh, "2 rows", refrain_scheme=[None, "AA"]).lines, pre, 4 * SENT, False)
    one = np.zeros(1 + 4 * SENT, bool)
    one[SENT + 1:SENT + 1 + CAP] = True
    assert got.tolist() == one.tolist()
    assert cols(None, None, 4 * SENT, False) is None and cols(_check_constraints(None, 0, 7, None, 2, 4 * SENT, sh, "2").lines, None, 4 * SENT,
                                                             False) is None
    dec._skips_copies = False
    assert cols(t, None, 4 * SENT, False) is None and BeamDecoder._skips_copies is False and GreedyDecoder._skips_copies is True
    dec._skips_copies = True
    monkeypatch.setenv("MMTG_DECODE_REFRAIN_SKIP", "0")
    assert cols(t, None, 4 * SENT, False) is None


# ------------------------------------------------------------------ the CPU restatement
class _Margins:
    """While active, records (lyric column, best - second best processed logit) of every column the restatements choose by arg-max
    (the outermost wrapper of test_lines_cpu.apply_rule: it sees the logits after every rule): test_beam_cpu.comparable_length of
    them is how far two fp32 computations of the ids can be held to each other."""

    def __init__(self):
        self.gaps = []

    def __call__(self, x, g, lo, hi, ends, sent=SENT):
        out = self.inner(x, g, lo, hi, ends, sent)
        if out is not None:
            top = torch.sort(out, descending=True).values[:2]
            self.gaps.append((len(g), float(top[0] - top[1]) if torch.isfinite(top[1]) else float("inf")))
        return out

    def __enter__(self):
        self.inner = L.apply_rule
        L.apply_rule = self
        return self

    def __exit__(self, *exc):
        L.apply_rule = self.inner


def cpu_refrain_greedy(w, sh, table, start, length, tables, b=0, n=0, prefix=(1,)):
    """Greedy decoding under every rule of tables' row b and its refrain: test_rhyme_cpu.cpu_rhyme_greedy up to each copy line, the
    copy column by column from the row's own ids (no logits, no bans; the held prefix and the cadence keep their columns), and on
    behind it with the ids so far as the prefix.  Returns (ids, gaps): the arg-max margins of the chosen columns, by column."""
    ids, gaps = [int(v) for v in prefix], []
    while len(ids) < length + 1:
        c = len(ids)
        l, q = c // SENT, c % SENT
        r = tables.source(b, l) if 0 < q < SENT - 1 else None
        if r is not None:
            ids.append(ids[c - (l - r) * SENT])
            continue
        stops = [m * SENT + 1 for m in range(l + 1, (length - 1) // SENT + 1) if tables.source(b, m) is not None]
        upto = min(stops + [length + 1])
        with _Margins() as m:
            ids, _ = cpu_rhyme_greedy(w, sh, table, start, upto - 1, tables, b=b, n=n, prefix=tuple(ids))
        gaps += m.gaps
    return ids, gaps


def lines_of(ids, sent=SENT):
    ids = [int(v) for v in ids]
    return [ids[l * sent + 1:l * sent + sent - 1] for l in range((len(ids) - 1) // sent)]


def copies_hold(ids, tables, b, start=1, sent=SENT):
    """Every copy column c >= start of row ids holds what the row holds at that column of the source line; returns how many."""
    ids = [int(v) for v in ids]
    count = 0
    for c in range(start, len(ids)):
        r = tables.source(b, c // sent) if 0 < c % sent < sent - 1 else None
        if r is not None:
            assert ids[c] == ids[c - (c // sent - r) * sent], (b, c)
            count += 1
    return count


def ngram_violations(ids, tables, b, n, start=1, sent=SENT):
    """The non-copy content columns c >= start of row ids that complete a content n-gram the FULL history before them holds (copied
    text included: the text after a copy cannot repeat it)."""
    ids = [int(v) for v in ids]
    return [c for c in range(start, len(ids))
            if 0 < c % sent < sent - 1 and tables.source(b, c // sent) is None and ids[c] != 0 and ids[c] in banned_ids(ids[:c], n)]


@pytest.mark.parametrize("row", [0, 1])
def test_schemes_under_which_nothing_repeats_reproduce_the_golden_ids(row):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    ref = fx["greedy_len220_row%d" % row].tolist()
    for scheme in ("..........", "ABCDEFGHIJ", ""):
        t = _check_constraints(None, 0, None, None, 1, 220, sh, "1 row", refrain_scheme=scheme).lines
        ids, _ = cpu_refrain_greedy(w, sh, table, start_row(batch, row), 220, t)
        assert GreedyDecoder.reference_return(ids, 220) == ref


@pytest.mark.parametrize("n", [0, 3])
def test_greedy_repeats_the_lines_of_the_scheme_also_under_ngram_blocking(n):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    tabs = _check_constraints(None, n, None, None, 2, LENGTH, sh, "2 rows", refrain_scheme=["AB.A", "AA.A"]).lines
    none = _check_constraints(None, n, (0, CAP), None, 2, LENGTH, sh, "2 rows").lines
    for row, first in ((0, 3), (1, 1)):
        ids, gaps = cpu_refrain_greedy(w, sh, table, start_row(batch, row), LENGTH, tabs, b=row, n=n)
        free, _ = cpu_rhyme_greedy(w, sh, table, start_row(batch, row), LENGTH, none, b=row, n=n)
        ln = lines_of(ids)
        assert len(ids) == LENGTH + 1 and ln[3] == ln[0] and any(ln[0]) and (row == 0 or ln[1] == ln[0])
        assert copies_hold(ids, tabs, row) == CAP * (1 if row == 0 else 2)
        assert ids[:first * SENT + 1] == free[:first * SENT + 1]               # the rule never touches a column before the first copy
        assert lines_of(free)[3] != lines_of(free)[0]                          # and without it the line does not come back
        assert n == 0 or ngram_violations(ids, tabs, row, n) == []
        assert [c for c, _ in gaps] == [c for c in range(1, LENGTH + 1) if 0 < c % SENT < SENT - 1 and tabs.source(row, c // SENT) is None
                                        and ids[c - 1] != 0]
    if n:                                                                       # what n-gram blocking alone does to a chorus: it cannot come back
        assert ngram_violations(ids, none, 1, n) != []                         # (read without the scheme, the copies ARE repeated n-grams)


def test_the_text_behind_a_copy_cannot_repeat_it():
    """Copied ids are ordinary history: under no_repeat_ngram_size the free line behind a copy is held against the copied text too."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    n = 2
    tabs = _check_constraints(None, n, None, None, 1, LENGTH, sh, "1 row", refrain_scheme="AA").lines
    ids, _ = cpu_refrain_greedy(w, sh, table, start_row(batch, 0), LENGTH, tabs, n=n)
    assert lines_of(ids)[1] == lines_of(ids)[0] and ngram_violations(ids, tabs, 0, n) == []
    grams = lambda xs: {tuple(xs[i:i + n]) for i in range(len(xs) - n + 1) if 0 not in xs[i:i + n]}     # noqa: E731
    assert not grams(lines_of(ids)[2]) & grams(lines_of(ids)[1])


@pytest.mark.parametrize("scheme,n", [("AAB.B", 0), ("AAB.B", 3), ("AA...", 3)])
def test_the_restatement_is_comparable_past_the_copy_line_in_every_fixture_row(scheme, n):
    """What tests/test_refrain_gpu.py's comparison with the decoder rests on: with the copy as line 1, no arg-max of the restatement
    is closer than comparable_length's 1e-4 before that line has ended -- here in none of the fixture's rows at all -- so the ids of
    two fp32 computations agree well past the copy.  Row 2 ends line 2 early: under "AAB.B" its copy repeats PADs."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    tabs = _check_constraints(None, n, None, None, 3, LENGTH, sh, "3 rows", refrain_scheme=scheme).lines
    for row in range(3):
        ids, gaps = cpu_refrain_greedy(w, sh, table, start_row(batch, row), LENGTH, tabs, b=row, n=n)
        assert comparable_length(gaps, LENGTH) == LENGTH > 2 * SENT - 1 and min(g for _, g in gaps) > 1e-4
        assert copies_hold(ids, tabs, row) == CAP * (2 if scheme == "AAB.B" else 1) and lines_of(ids)[1] == lines_of(ids)[0]
    if scheme == "AAB.B":
        assert 0 in lines_of(ids)[2] and any(lines_of(ids)[2]) and lines_of(ids)[4] == lines_of(ids)[2]
