"""Classifier-free guidance on the host: the float64 restatement (constraints.guidance_scores) against transformers'
ClassifierFreeGuidanceLogitsProcessor on log-softmaxed rows and its own properties; the range check of the Python surface and the
argument checks of both C entries; the header, the bindings and the exports; `cpu_guided_greedy`, the guided greedy search restated on
the committed oracle, and the check on that yardstick itself; the float32 transcription of the kernel (tools/guidance_fp32_bands.py)
inside the band tests/test_guidance_gpu.py holds the device to, and four planted defects outside it.  No GPU: a bad argument fails
before any device call.

The band.  |device - float64| <= K * 2^-24 * (1 + 2 s) * M per pair, M = max(|c|inf + |L(c)|, |u|inf + |L(u)|).  The tool's transcription
(the kernel's order of operations in float32 numpy) has a worst k of 1.44 over V = 257 / 500 / 13317, three value scales, both load
paths, the five scales and three seeds; K is twice that rounded up to an integer, 3: the factor 2 covers the device's expf / logf,
its fused multiply-adds and its reduction order, which the transcription only approximates."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.constraints import GUIDANCE_OFF, _log_softmax64, check_guidance, guidance_scores
from mmtg_amd.decode import GuidedDecoder
from oracle import mmtg_oracle as O
from test_beam_cpu import SENT, setup_case, start_row
from test_prefix_cpu import REP, T
from test_warp_cpu import rows_for

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = (0.0, 1.0, 1.5, 3.0, 7.5)
K_BAND = 3

_spec = importlib.util.spec_from_file_location("guidance_fp32_bands", os.path.join(HERE, "..", "tools", "guidance_fp32_bands.py"))
bands = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bands)


def lsm(x):
    return torch.log_softmax(torch.from_numpy(np.asarray(x, dtype=np.float64)), -1).numpy()


def pairs_for(seed, V=500):
    """(c, u) pairs of the kinds the tests use: random rows at scales 1 / 3 / 6, rows with -inf holes (in c only, in u only, in both),
    a one-hot row against a random one, a uniform row against a random one."""
    r, q = rows_for(seed, V), rows_for(seed + 100, V)
    rng = np.random.default_rng(seed + 7)
    both = q[3].copy()
    both[np.isneginf(r[3])] = -np.inf
    return [(r[0], q[0]), (r[1], q[1]), (r[2], q[2]), (r[3], q[1]), (r[1], q[3]), (r[3], both), (r[5], q[0]), (q[0], r[5]),
            (r[7], q[1]), (r[1], rng.normal(size=V) * 3.0)]


# ------------------------------------------------------------------ 1. the restatement against transformers
def hf_guided(c, u, s):
    """transformers' batched processor on the float64 log-softmaxed rows [c; u], as its unbatched form runs it.  Its constructor
    refuses a scale <= 1 (generate has no use for one); the scale is an attribute and __call__ is the rule at any value, so the
    processor is built at 2 and told the scale."""
    from transformers.generation import logits_process as lp
    proc = lp.ClassifierFreeGuidanceLogitsProcessor(2.0)
    proc.guidance_scale = s
    scores = torch.from_numpy(np.stack([lsm(c), lsm(u)]))
    return proc(torch.zeros(1, 1, dtype=torch.long), scores)[0].numpy()


@pytest.mark.parametrize("s", SCALES)
def test_the_restatement_is_transformers_guidance_on_log_softmaxed_rows(s):
    seen = 0
    for seed in range(3):
        for c, u in pairs_for(seed):
            got = guidance_scores(c, u, s)
            with np.errstate(invalid="ignore"):
                want = hf_guided(c, u, s)
            fin = np.isfinite(c) & np.isfinite(u)
            # (transformers leaves NaN where both rows exclude an id, and at scale 0 where the prompt alone does: 0 * -inf; the rule here is -inf)
            assert np.array_equal(np.isfinite(got), fin) and bool(np.isneginf(got[~fin]).all())
            assert fin.any() and np.abs(got[fin] - want[fin]).max() <= 1e-12 * (1 + 2 * s) * np.abs(want[fin]).max()
            seen += 1
    assert seen == 30


def test_the_properties_of_the_rule():
    for seed in range(3):
        for c, u in pairs_for(seed):
            fin = np.isfinite(c) & np.isfinite(u)
            one, zero = guidance_scores(c, u, 1.0), guidance_scores(c, u, 0.0)
            assert np.abs(one[fin] - lsm(c)[fin]).max() <= 1e-12 and np.abs(zero[fin] - lsm(u)[fin]).max() <= 1e-12
            for s in SCALES:
                same = guidance_scores(c, c, s)
                assert np.array_equal(same, _log_softmax64(np.asarray(c, np.float64)))          # c == u: lsm(c) exactly, whatever the scale
                assert np.abs(same[np.isfinite(c)] - lsm(c)[np.isfinite(c)]).max() <= 1e-12     # (torch's, to rounding)
                g = guidance_scores(c, u, s)
                assert not np.isnan(g).any() and bool((g[fin] <= 1e-9).all() or s > 1.0)
                shifted = guidance_scores(np.asarray(c) + 3.25, np.asarray(u) - 11.5, s)         # a per-row shift changes nothing
                assert np.array_equal(np.isfinite(shifted), fin)
                assert np.abs(shifted[fin] - g[fin]).max() <= 1e-11 * (1 + 2 * s)
    V = 64
    dead = np.full(V, -np.inf)
    live = np.random.default_rng(0).normal(size=V)
    for s in SCALES:
        for c, u in ((dead, live), (live, dead), (dead, dead)):
            assert bool(np.isneginf(guidance_scores(c, u, s)).all())                              # a row without a distribution
    batched = guidance_scores(np.stack([live, dead]), np.stack([live * 2, live]), 3.0)
    assert batched.shape == (2, V) and np.array_equal(batched[0], guidance_scores(live, live * 2, 3.0)) and bool(np.isneginf(batched[1]).all())
    with pytest.raises(ValueError, match="shape"):
        guidance_scores(live, live[:-1], 2.0)


# ------------------------------------------------------------------ 2. argument checks and plumbing
def test_check_guidance_takes_finite_numbers_from_zero_up_and_names_the_argument():
    assert GUIDANCE_OFF == 1.0 and check_guidance() == 1.0
    assert check_guidance(0) == 0.0 and check_guidance(np.float32(1.5)) == 1.5 and check_guidance(7.5) == 7.5 and check_guidance(3) == 3.0
    for bad in (True, False, "3.0", b"3", None, float("nan"), float("inf"), -float("inf"), -0.5, [2.0]):
        with pytest.raises(ValueError, match="guidance_scale"):
            check_guidance(bad)
    with pytest.raises(ValueError, match="guidance_scale"):
        guidance_scores(np.zeros(4), np.zeros(4), -1.0)


def _guidance_args(cond=0x7000000000, uncond=0x7100000000, ldl=16, V=16, scale=3.0, out=0x7200000000, ldo=16, N=4):
    p = lambda a: None if a is None else C.c_void_p(a)          # never dereferenced: the checks come before any device call
    return (p(cond), p(uncond), ldl, V, scale, p(out), ldo, N, None)


def _mirror_args(seq=0x7000000000, ldseq=64, pos=0x7100000000, N=4):
    p = lambda a: None if a is None else C.c_void_p(a)
    return (p(seq), ldseq, p(pos), N, None)


def test_both_c_entries_return_minus_one_with_the_arguments_name_before_any_device_call():
    L = hip.lib()
    base = 0x7200000000
    bad = [("cond", dict(cond=None)), ("uncond", dict(uncond=None)), ("out", dict(out=None)), ("N", dict(N=0)), ("N", dict(N=-3)),
           ("V", dict(V=0)), ("ldl", dict(ldl=15)), ("ldo", dict(ldo=15)), ("scale", dict(scale=float("nan"))),
           ("scale", dict(scale=float("inf"))), ("scale", dict(scale=-0.5)),
           ("out overlaps cond", dict(cond=base)), ("out overlaps cond", dict(cond=base + 4 * (3 * 16 + 15))),       # its last element
           ("out overlaps cond", dict(cond=base - 4 * (3 * 16 + 15))), ("out overlaps uncond", dict(uncond=base + 64)),
           ("out overlaps uncond", dict(uncond=base))]
    for word, kw in bad:
        assert L.mmtg_decode_guidance(*_guidance_args(**kw)) == -1, kw
        msg = L.mmtg_last_error().decode()
        assert msg.startswith("decode_guidance: ") and re.search(r"\b%s\b" % word, msg), (kw, msg)
    for word, kw in [("seq", dict(seq=None)), ("pos_ptr", dict(pos=None)), ("N", dict(N=0)), ("ldseq", dict(ldseq=0))]:
        assert L.mmtg_decode_mirror(*_mirror_args(**kw)) == -1, kw
        msg = L.mmtg_last_error().decode()
        assert msg.startswith("decode_mirror: ") and re.search(r"\b%s\b" % word, msg), (kw, msg)
    # the Python wrappers check what they can see
    with pytest.raises(ValueError, match="fp32"):
        hip.decode_guidance(torch.zeros(4, dtype=torch.float64), torch.zeros(4), 4, 4, 2.0, torch.zeros(1, 4), 1)
    with pytest.raises(ValueError, match="int64"):
        hip.decode_mirror(torch.zeros(2, 8, dtype=torch.int32), None, 1)
    with pytest.raises(ValueError, match="2 N"):
        hip.decode_mirror(torch.zeros(3, 8, dtype=torch.long), None, 2)


def test_the_entries_are_declared_bound_and_exported_and_the_abi_version_is_12():
    header = open(os.path.join(HERE, "..", "include", "mmtg_hip.h")).read()
    for name, n_args in (("mmtg_decode_guidance", 9), ("mmtg_decode_mirror", 5)):
        assert re.search(r"MMTG_API int %s\(" % name, header)
        assert name in hip.exported_symbols() and hasattr(C.CDLL(hip.lib_path()), name)
        assert getattr(hip.lib(), name).restype is C.c_int and len(hip._SIGS[name][0]) == n_args
    assert hip._SIGS["mmtg_decode_guidance"][0][4] is C.c_float
    for word in ("lu + scale * (lc - lu)", "UnbatchedClassifierFreeGuidanceLogitsProcessor", "seq[(N + b) * ldseq + pos + 1]"):
        assert word in header
    assert "#define MMTG_ABI_VERSION 12" in header and hip.ABI_VERSION == 12 and hip.lib().mmtg_abi_version() == 12
    assert callable(hip.decode_guidance) and callable(hip.decode_mirror)


def test_the_surface_refuses_a_negative_without_a_scale_and_more_than_one_lane():
    from mmtg_amd.generate import generate_samples, sample_sequence, without_experience
    with pytest.raises(ValueError, match="negative_rows"):
        generate_samples(None, [], None, guidance_scale=1.0, negative_rows=[])
    with pytest.raises(ValueError, match="negative_input"):
        sample_sequence(None, {}, 8, None, guidance_scale=1, negative_input={})
    for bad in (-1.0, float("nan"), "3", None, True):
        with pytest.raises(ValueError, match="guidance_scale"):
            generate_samples(None, [], None, guidance_scale=bad)
        with pytest.raises(ValueError, match="guidance_scale"):
            sample_sequence(None, {}, 8, None, guidance_scale=bad)
        with pytest.raises(ValueError, match="guidance_scale"):
            GuidedDecoder.begin(None, {"img_embs": np.zeros((1, 1))}, {"img_embs": np.zeros((1, 1))}, 8, guidance_scale=bad)
    with pytest.raises(ValueError, match="one lane"):
        GuidedDecoder(None, 2, lanes=2)
    import inspect
    from mmtg_amd.generate import generate_beams, generate_contrastive
    for fn in (generate_beams, generate_contrastive):                          # out of scope: the merge reorders what a column mirror cannot follow
        assert "guidance_scale" not in inspect.signature(fn).parameters
    for fn, neg in ((generate_samples, "negative_rows"), (sample_sequence, "negative_input")):
        p = inspect.signature(fn).parameters
        assert p["guidance_scale"].kind is p[neg].kind is inspect.Parameter.KEYWORD_ONLY and p["guidance_scale"].default == 1.0
    rows = {"topic_ids": np.ones((2, 3), np.int64), "tpw_attention_mask": np.ones((2, 3), np.int64), "tpw_type_ids": np.ones((2, 3), np.int64),
            "topic_emb": np.ones((2, 4), np.float32), "img_embs": np.ones((2, 5, 4), np.float32), "r_embs": np.ones((2, 5, 4), np.float32)}
    neg = without_experience(rows)
    assert float(neg["img_embs"].abs().sum()) == 0 and float(neg["r_embs"].abs().sum()) == 0 and neg["img_embs"].shape == (2, 5, 4)
    for k in ("topic_ids", "tpw_attention_mask", "tpw_type_ids", "topic_emb"):
        assert np.array_equal(neg[k].numpy(), rows[k])
    assert float(rows["img_embs"].sum()) == 40.0                                # the caller's rows are left alone


# ------------------------------------------------------------------ 3. the guided greedy search on the oracle
def zeroed(start):
    return {k: (np.zeros_like(v) if k in ("img_embs", "r_embs") else v) for k, v in start.items()}


def cpu_guided_greedy(w, sh, table, start, negative, length, scale, temperature, repetition_penalty, margins=None):
    """One prompt (`start`) and its negative (`negative`: dataset rows without targets), the reference loop's cadence
    (generate.py:117-142), two cached forwards.  At every model call the guided scores of the two last rows (guidance_scores, float64,
    cut at 13317) take the logits' place in process_logits; the pick is the lowest arg-max.  Returns the 1 + length lyric ids;
    margins (a list, optional) receives (lyric column, top-2 margin of the processed scores) per model call."""
    def base(row):
        b = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in row.items() if k not in ("targets", "rating")}
        b["topic_ids"] = b["topic_ids"].long()
        return b
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    sides = [(O.CachedForward(w, sh, table), base(start)), (O.CachedForward(w, sh, table), base(negative))]
    ids = [1]
    for i in range(length):
        if i > 0 and (i + 2) % SENT in (0, 1):
            ids.append(2 if (i + 2) % SENT == 0 else 1)
            continue
        c, u = (cf(dict(b, targets=torch.tensor([ids], dtype=torch.long)))[0, -1, :V].double().numpy() for cf, b in sides)
        if ids[-1] == 0:
            ids.append(0)
            continue
        x = O.process_logits(torch.from_numpy(guidance_scores(c, u, scale)), torch.tensor(ids), temperature, repetition_penalty)
        top = torch.sort(x, descending=True, stable=True)
        if margins is not None:
            margins.append((len(ids), float(top.values[0] - top.values[1])))
        ids.append(int(top.indices[0]))
    return ids


@pytest.mark.parametrize("case", ["tiny_s5", "tiny_s2"])
def test_the_guided_search_at_scale_one_without_a_penalty_is_the_oracles_greedy_search(case):
    """The check on the yardstick itself: log-softmax keeps the order, the temperature and the bans keep it too, so at scale 1 and
    penalty 1 any negative leaves the oracle's own greedy ids; the per-occurrence penalty divides whatever number it finds, a
    log-probability here and a raw logit there, so at penalty 1.5 the texts part."""
    fx, sh, w, table, batch = setup_case(case)
    length = 3 * SENT
    B = batch["topic_ids"].shape[0]
    start = start_row(batch, 0)
    plain = {rep: O.sample_sequence(O.CachedForward(w, sh, table), dict(start, targets=np.array([1])), length, temperature=T, top_k=1,
                                    top_p=0.0, repitition_penalty=rep, greedy=True) for rep in (1.0, REP)}
    for negative in (start_row(batch, 1 % B), zeroed(start)):
        got = cpu_guided_greedy(w, sh, table, start, negative, length, 1.0, T, 1.0)
        assert got[:len(plain[1.0])] == plain[1.0] and len(got) == 1 + length
    got = cpu_guided_greedy(w, sh, table, start, zeroed(start), length, 1.0, T, REP)
    assert got[:len(plain[REP])] != plain[REP]
    guided = cpu_guided_greedy(w, sh, table, start, zeroed(start), length, 3.0, T, 1.0)
    assert guided[:len(plain[1.0])] != plain[1.0]                               # and a scale steers


# ------------------------------------------------------------------ 4. the transcription, the band and four planted defects
def float64_of(c, u, s, V):
    return guidance_scores(np.asarray(c, np.float32)[:V], np.asarray(u, np.float32)[:V], s)


def band_of(c, u, s, V):
    return K_BAND * bands.band_unit(np.asarray(c, np.float32)[:V], np.asarray(u, np.float32)[:V], s)


def padded_pairs(seed, V, Vpad):
    """pairs_for's rows in float32 with columns V .. Vpad - 1 filled with large finite values the rule must not read."""
    out = []
    for c, u in pairs_for(seed, V):
        cp, up = np.full(Vpad, 40.0, np.float32), np.full(Vpad, 38.0, np.float32)
        cp[:V], up[:V] = c, u
        out.append((cp, up))
    return out


def test_the_transcription_of_the_kernel_lies_inside_the_band_on_both_load_paths():
    worst = 0.0
    for V, Vpad in ((257, 264), (500, 512)):
        for c, u in padded_pairs(1, V, Vpad):
            for s in SCALES:
                want = float64_of(c, u, s, V)
                fin = np.isfinite(want)
                if not fin.any():
                    continue
                for aligned in (True, False):
                    got = bands.kernel_f32(c, u, s, aligned, V=V).astype(np.float64)
                    assert np.array_equal(np.isfinite(got), fin) and bool(np.isneginf(got[~fin]).all())
                    worst = max(worst, float(np.abs(got[fin] - want[fin]).max() / band_of(c, u, s, V)))
    print("worst error of the float32 transcription: %.3f of the band" % worst)
    assert worst <= 0.5                                                         # K is twice the transcription's worst, rounded up
    c = np.random.default_rng(4).normal(size=500).astype(np.float32)
    for s in SCALES:                                                            # c == u: lu bit for bit at any scale
        assert np.array_equal(bands.kernel_f32(c, c, s), bands.kernel_f32(c, c, 0.0))


def _defect(name, c, u, s, V):
    f = np.float32
    c, u = np.asarray(c, f), np.asarray(u, f)
    if name == "lse over Vpad":
        Lc, Lu = bands.row_lse(c), bands.row_lse(u)
    else:
        Lc, Lu = bands.row_lse(c[:V]), bands.row_lse(u[:V])
    c, u = c[:V], u[:V]
    if name == "halves swapped":
        c, u, Lc, Lu = u, c, Lu, Lc
    with np.errstate(invalid="ignore"):
        lc, lu = (c - Lc).astype(f), ((u - Lu).astype(f) if name != "u unnormalised" else u)
        g = (lu + f(s) * lc).astype(f) if name == "s * lc + lu" else (lu + f(s) * (lc - lu).astype(f)).astype(f)
    return np.where(np.isneginf(c) | np.isneginf(u), f(-np.inf), g).astype(np.float64)


@pytest.mark.parametrize("name", ["lse over Vpad", "u unnormalised", "halves swapped", "s * lc + lu"])
def test_a_planted_defect_exceeds_the_band(name):
    """Each defect in the float32 transcription leaves the band on every random pair, at every scale that lets it show (swapped halves
    are invisible at c == u only; s * lc + lu equals the rule at s = 0; an unnormalised u is invisible at s = 1, where u drops out
    up to rounding)."""
    V, Vpad = 500, 512
    hidden = {"u unnormalised": (1.0,), "s * lc + lu": (0.0,)}.get(name, ())
    shown = 0
    for c, u in padded_pairs(2, V, Vpad)[:3]:
        for s in SCALES:
            if s in hidden:
                continue
            want = float64_of(c, u, s, V)
            err = float(np.abs(_defect(name, c, u, s, V) - want).max())
            assert err > band_of(c, u, s, V), (name, s, err, band_of(c, u, s, V))
            shown += 1
        ok = bands.kernel_f32(c, u, 3.0, V=V).astype(np.float64)
        assert float(np.abs(ok - float64_of(c, u, 3.0, V)).max()) <= band_of(c, u, 3.0, V)
    assert shown >= 12
