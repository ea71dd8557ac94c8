"""Per-modality guidance on the host: the float64 restatement of the rule (constraints.modality_guidance_scores) and its properties;
the branch check; the argument checks of the C entries, which fail before any device call (the library loads without a GPU, as
tests/test_guidance_cpu.py shows); the bindings, the header and the exports; the surface's argument errors and the chunk size.  The
allowance of the kernel tests (tests/mg_ref.py) is checked here for what it can be checked for without a device: it is positive,
it grows with the scales, and a planted defect leaves it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mg_ref
from mmtg_amd import hip
from mmtg_amd.constraints import (GUIDANCE_BRANCHES, _log_softmax64, check_modality_guidance, guidance_scores,
                                  modality_guidance_scores)
from mmtg_amd.decode import GuidedDecoder, ModalityGuidedDecoder
from test_guidance_cpu import pairs_for

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = (0.0, 0.5, 1.0, 1.5, 3.0, 7.5)
NINF = float("-inf")


# ------------------------------------------------------------------ 1. the float64 rule
def test_all_scales_at_one_give_the_prompts_log_softmax():
    for seed in range(3):
        for c, u in pairs_for(seed):
            lc = _log_softmax64(np.asarray(c, np.float64))
            for K in (1, 2, 3, 4):
                fin = np.isfinite(c) & (np.isfinite(u) if K > 1 else True)
                g = modality_guidance_scores([c] + [u] * (K - 1), [1.0] * (K - 1))
                assert np.array_equal(g[fin], lc[fin]) and bool(np.isneginf(g[~fin]).all())


def test_one_branch_is_guidance_scores():
    for seed in range(3):
        for c, u in pairs_for(seed):
            for s in SCALES:
                got, want = modality_guidance_scores([c, u], [s]), guidance_scores(c, u, s)
                fin = np.isfinite(want)
                assert np.array_equal(np.isfinite(got), fin) and bool(np.isneginf(got[~fin]).all())
                if fin.any():       # lc + (s - 1)(lc - lu) against lu + s (lc - lu): the same number up to float64 rounding
                    assert np.abs(got[fin] - want[fin]).max() <= 1e-12 * (1 + 2 * s) * max(1.0, np.abs(want[fin]).max())


def test_a_branch_equal_to_the_prompt_vanishes_at_any_scale():
    rng = np.random.default_rng(5)
    c, u, t = (rng.normal(size=300) * 3.0 for _ in range(3))
    for s in SCALES:
        assert np.array_equal(modality_guidance_scores([c, c], [s]), _log_softmax64(c))
        for other in SCALES:
            assert np.array_equal(modality_guidance_scores([c, u, c], [other, s]), modality_guidance_scores([c, u], [other]))
            assert np.array_equal(modality_guidance_scores([c, c, u, t], [s, other, 3.0]), modality_guidance_scores([c, u, t], [other, 3.0]))


def test_minus_infinity_in_any_branch_excludes_the_id_and_an_empty_row_excludes_every_id():
    rng = np.random.default_rng(6)
    V = 64
    rows = [rng.normal(size=V) for _ in range(4)]
    for K in (2, 3, 4):
        for k in range(K):
            for scales in ([0.0] * (K - 1), [3.0, 1.5, 0.5][:K - 1], [7.5] * (K - 1)):
                x = [r.copy() for r in rows[:K]]
                x[k][5] = NINF
                g = modality_guidance_scores(x, scales)
                assert not np.isnan(g).any() and np.isneginf(g[5]) and bool(np.isfinite(np.delete(g, 5)).all())
                x[k][:] = NINF
                g = modality_guidance_scores(x, scales)
                assert bool(np.isneginf(g).all())
    batched = modality_guidance_scores(np.stack([np.stack([rows[0], rows[1]]), np.stack([rows[2], np.full(V, NINF)])]), [3.0])
    assert batched.shape == (2, V) and np.array_equal(batched[0], modality_guidance_scores([rows[0], rows[2]], [3.0]))
    assert bool(np.isneginf(batched[1]).all())
    with pytest.raises(ValueError, match="scales"):
        modality_guidance_scores([rows[0], rows[1]], [2.0, 3.0])
    with pytest.raises(ValueError, match="shape"):
        modality_guidance_scores([rows[0], rows[1][:-1]], [2.0])
    with pytest.raises(ValueError, match="guidance_scale"):
        modality_guidance_scores([rows[0], rows[1]], [-1.0])


def test_the_weight_on_the_prompt_may_be_negative():
    rng = np.random.default_rng(8)
    c, u, i, t = (rng.normal(size=50) for _ in range(4))
    g = modality_guidance_scores([c, u, i, t], [0.0, 0.0, 0.0])
    want = -2.0 * _log_softmax64(c) + _log_softmax64(u) + _log_softmax64(i) + _log_softmax64(t)
    assert bool(np.isfinite(g).all()) and np.abs(g - want).max() <= 1e-12


def test_check_modality_guidance_returns_the_running_branches_in_order_and_names_the_bad_argument():
    assert GUIDANCE_BRANCHES == ("u", "i", "t")
    assert check_modality_guidance() == ((), ()) and check_modality_guidance(1, 1.0, np.float32(1.0)) == ((), ())
    assert check_modality_guidance(3.0) == (("u",), (3.0,))
    assert check_modality_guidance(image_guidance_scale=3) == (("i",), (3.0,))
    assert check_modality_guidance(1.0, 3.0, 1.5) == (("i", "t"), (3.0, 1.5))
    assert check_modality_guidance(0, 1.0, 0.5) == (("u", "t"), (0.0, 0.5))
    assert check_modality_guidance(2.0, 3.0, 1.5) == (("u", "i", "t"), (2.0, 3.0, 1.5))
    names = ("guidance_scale", "image_guidance_scale", "text_guidance_scale")
    for at, name in enumerate(names):
        for bad in (True, "3.0", None, float("nan"), float("inf"), -0.5, [2.0]):
            args = [2.0, 2.0, 2.0]
            args[at] = bad
            with pytest.raises(ValueError) as e:
                check_modality_guidance(*args)
            assert str(e.value).startswith(name + " must be"), (name, str(e.value))


# ------------------------------------------------------------------ 2. the C entries and the bindings
def _multi_args(logits=0x7000000000, ldl=16, V=16, K=3, scales=(3.0, 1.5, 1.0), out=0x7200000000, ldo=16, N=4):
    p = lambda a: None if a is None else C.c_void_p(a)          # never dereferenced: the checks come before any device call
    host = None if scales is None else (C.c_float * 3)(*scales)
    return (p(logits), ldl, V, K, host, p(out), ldo, N, None)


def _mirror_args(seq=0x7000000000, ldseq=64, pos=0x7100000000, N=4, K=3):
    p = lambda a: None if a is None else C.c_void_p(a)
    return (p(seq), ldseq, p(pos), N, K, None)


def test_every_refusal_returns_minus_one_with_the_entry_and_the_argument_before_any_device_call():
    L = hip.lib()
    out = 0x7200000000
    rows = 3 * 4            # K N input rows of 16 floats
    bad = [("logits", dict(logits=None)), ("scales", dict(scales=None)), ("out", dict(out=None)), ("N", dict(N=0)), ("N", dict(N=-3)),
           ("V", dict(V=0)), ("K", dict(K=1)), ("K", dict(K=5)), ("K", dict(K=0)), ("ldl", dict(ldl=15)), ("ldo", dict(ldo=15)),
           ("scale", dict(scales=(float("nan"), 1.0, 1.0))), ("scale", dict(scales=(3.0, float("inf"), 1.0))),
           ("scale", dict(scales=(3.0, -0.5, 1.0))), ("scale", dict(K=4, scales=(3.0, 1.5, -1.0))),
           ("out overlaps logits", dict(logits=out)), ("out overlaps logits", dict(logits=out + 4 * (3 * 16 + 15))),    # out's last element
           ("out overlaps logits", dict(logits=out - 4 * (rows * 16 - 1))),                                             # the inputs' last element
           ("out overlaps logits", dict(logits=out - 4 * 16 * 5))]                                                      # a row of block 1
    for word, kw in bad:
        assert L.mmtg_decode_guidance_multi(*_multi_args(**kw)) == -1, kw
        msg = L.mmtg_last_error().decode()
        assert msg.startswith("decode_guidance_multi: ") and re.search(r"\b%s\b" % word, msg), (kw, msg)
    assert hip._SIGS["mmtg_decode_guidance_multi"][0][4] is C.c_void_p          # the scales travel as a host pointer
    for word, kw in [("form", dict(form=3)), ("form", dict(form=-1)), ("V", dict(form=1, V=14337, ldl=14337, ldo=14337))]:
        form = kw.pop("form")
        a = _multi_args(**kw)
        assert L.mmtg_decode_guidance_multi_form(*a[:-1], form, None) == -1
        msg = L.mmtg_last_error().decode()
        assert msg.startswith("decode_guidance_multi_form: ") and re.search(r"\b%s\b" % word, msg), (kw, msg)
    for word, kw in [("seq", dict(seq=None)), ("pos_ptr", dict(pos=None)), ("N", dict(N=0)), ("K", dict(K=1)), ("K", dict(K=5)),
                     ("ldseq", dict(ldseq=0))]:
        assert L.mmtg_decode_mirror_multi(*_mirror_args(**kw)) == -1, kw
        msg = L.mmtg_last_error().decode()
        assert msg.startswith("decode_mirror_multi: ") and re.search(r"\b%s\b" % word, msg), (kw, msg)


def test_the_bindings_check_dtype_and_layout():
    f32 = torch.zeros(6, 8)
    with pytest.raises(ValueError, match="fp32"):
        hip.decode_guidance_multi(f32.double(), 8, 8, (3.0, 1.5), torch.zeros(2, 8), 2)
    with pytest.raises(ValueError, match="fp32"):
        hip.decode_guidance_multi(f32, 8, 8, (3.0, 1.5), torch.zeros(2, 8, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="K N"):
        hip.decode_guidance_multi(f32, 8, 8, (3.0, 1.5, 2.0), torch.zeros(2, 8), 2)            # 8 rows wanted, 6 there
    with pytest.raises(ValueError, match="ldl"):
        hip.decode_guidance_multi(f32, 4, 4, (3.0, 1.5), torch.zeros(2, 8), 2)                 # the rows are 8 apart
    with pytest.raises(ValueError, match="column stride"):
        hip.decode_guidance_multi(f32, 8, 8, (3.0, 1.5), torch.zeros(8, 2).t(), 2)
    with pytest.raises(ValueError, match="form"):
        hip.decode_guidance_multi(f32, 8, 8, (3.0, 1.5), torch.zeros(2, 8), 2, form="fastest")
    with pytest.raises(ValueError, match="int64"):
        hip.decode_mirror_multi(torch.zeros(6, 8, dtype=torch.int32), None, 2, 3)
    with pytest.raises(ValueError, match="K N"):
        hip.decode_mirror_multi(torch.zeros(5, 8, dtype=torch.long), None, 2, 3)


def test_the_entries_are_declared_bound_and_exported_and_the_abi_version_is_12():
    header = open(os.path.join(HERE, "..", "include", "mmtg_hip.h")).read()
    for name, n_args in (("mmtg_decode_guidance_multi", 9), ("mmtg_decode_guidance_multi_form", 10), ("mmtg_decode_mirror_multi", 6)):
        assert re.search(r"MMTG_API int %s\(" % name, header)
        assert name in hip.exported_symbols() and hasattr(C.CDLL(hip.lib_path()), name)
        assert getattr(hip.lib(), name).restype is C.c_int and len(hip._SIGS[name][0]) == n_args
    for word in ("g = g + w_k * (lc - l_k)", "seq[(k N + b) * ldseq + pos + 1]", "handed to the kernel by value"):
        assert word in header
    assert "global: mmtg_*;" in open(os.path.join(HERE, "..", "mmtg_amd", "csrc", "exports.map")).read()
    assert "#define MMTG_ABI_VERSION 12" in header and hip.ABI_VERSION == 12 and hip.lib().mmtg_abi_version() == 12
    assert callable(hip.decode_guidance_multi) and callable(hip.decode_mirror_multi)


# ------------------------------------------------------------------ 3. the surface
def test_the_surface_refuses_bad_scales_a_negative_without_its_scale_and_the_rerun_loop_with_two_branches():
    from mmtg_amd.generate import generate_beams, generate_contrastive, generate_samples, generate_stochastic_beams, sample_sequence
    for name in ("image_guidance_scale", "text_guidance_scale"):
        for bad in (-1.0, float("nan"), "3", None, True):
            with pytest.raises(ValueError, match="^" + name):
                generate_samples(None, [], None, **{name: bad})
            with pytest.raises(ValueError, match="^" + name):
                sample_sequence(None, {}, 8, None, **{name: bad})
    # negative_rows / negative_input replace the u branch only: beside guidance_scale = 1 they are refused, whatever the other scales
    with pytest.raises(ValueError, match="negative_rows"):
        generate_samples(None, [], None, guidance_scale=1.0, image_guidance_scale=3.0, negative_rows=[])
    with pytest.raises(ValueError, match="negative_input"):
        sample_sequence(None, {}, 8, None, image_guidance_scale=3.0, text_guidance_scale=1.5, negative_input={})
    # no cached decoder for this call (no model): the re-run loop would run, and it takes one negative
    with pytest.raises(ValueError, match="re-run loop"):
        sample_sequence(None, {"targets": np.asarray([1])}, 8, None, image_guidance_scale=3.0, text_guidance_scale=1.5)
    with pytest.raises(ValueError, match="re-run loop"):
        sample_sequence(None, {"targets": np.asarray([1])}, 8, None, guidance_scale=2.0, image_guidance_scale=3.0, text_guidance_scale=1.5)
    for fn in (generate_samples, sample_sequence):
        p = inspect.signature(fn).parameters
        for name in ("image_guidance_scale", "text_guidance_scale"):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == 1.0
    for fn in (generate_beams, generate_contrastive, generate_stochastic_beams):        # the searches take no guidance, as before
        assert not any("guidance" in name for name in inspect.signature(fn).parameters)
    with pytest.raises(ValueError, match="one lane"):
        ModalityGuidedDecoder(None, 2, 3, lanes=2)
    for blocks in (1, 5):
        with pytest.raises(ValueError, match="blocks"):
            ModalityGuidedDecoder(None, 2, blocks)
    assert issubclass(ModalityGuidedDecoder, GuidedDecoder)
    with pytest.raises(ValueError, match="guidance_scale"):
        ModalityGuidedDecoder.begin(None, {}, [{}, {}], 8, ("i", "t"), (3.0, -1.0))


def test_without_images_and_without_texts_zero_one_channel_each_and_leave_the_rows_alone():
    from mmtg_amd.generate import without_experience, without_images, without_texts
    rows = {"topic_ids": np.ones((2, 3), np.int64), "tpw_attention_mask": np.ones((2, 3), np.int64), "tpw_type_ids": np.ones((2, 3), np.int64),
            "topic_emb": np.ones((2, 4), np.float32), "img_embs": np.ones((2, 5, 4), np.float32), "r_embs": np.ones((2, 5, 4), np.float32)}
    ni, nt, nu = without_images(rows), without_texts(rows), without_experience(rows)
    assert float(ni["img_embs"].abs().sum()) == 0 and float(ni["r_embs"].sum()) == 40.0
    assert float(nt["r_embs"].abs().sum()) == 0 and float(nt["img_embs"].sum()) == 40.0
    assert float(nu["img_embs"].abs().sum()) == 0 and float(nu["r_embs"].abs().sum()) == 0
    for neg in (ni, nt):
        for k in ("topic_ids", "tpw_attention_mask", "tpw_type_ids", "topic_emb"):
            assert np.array_equal(neg[k].numpy(), rows[k])
    assert float(rows["img_embs"].sum()) == 40.0 and float(rows["r_embs"].sum()) == 40.0
    items = [{k: v[b] for k, v in rows.items()} for b in range(2)]              # a list of dataset items works too
    assert without_images(items)["img_embs"].shape == (2, 5, 4)


def test_a_guided_chunk_holds_max_batch_over_k_prompts():
    from mmtg_amd.generate import guided_chunk_size
    assert [guided_chunk_size(256, K, 10 ** 6) for K in (2, 3, 4)] == [128, 85, 64]
    assert guided_chunk_size(256, 3, 6) == 6 and guided_chunk_size(2, 3, 6) == 1 and guided_chunk_size(7, 4, 100) == 1
    assert guided_chunk_size(8, 4, 100) == 2


# ------------------------------------------------------------------ 4. the allowance of the kernel tests
def test_the_allowance_is_positive_grows_with_the_scales_and_a_planted_defect_leaves_it():
    V, K, N = 257, 3, 3
    x = mg_ref.case(V, K, N)
    assert x.shape == (K, N, V) and np.isneginf(x[1, 0, V // 2]) and bool(np.isneginf(x[K - 1, N - 1]).all())
    small, big = mg_ref.multi_allow(x, (1.5, 0.5)), mg_ref.multi_allow(x, (7.5, 3.0))
    assert small[N - 1] == 0 and big[N - 1] == 0                                 # the prompt without a distribution: -inf exactly
    assert bool((small[:N - 1] > 0).all()) and bool((big[:N - 1] > small[:N - 1]).all()) and bool((big < 1e-2).all())
    want, allow = mg_ref.reference(V, K, N, (3.0, 1.5))
    assert bool(np.isneginf(want[N - 1]).all()) and np.isneginf(want[0, V // 2]) and bool(np.isfinite(np.delete(want[0], V // 2)).all())
    # float32 evaluation of the rule on float64 log-softmaxes lies inside; the log-sum-exp taken over the padding does not
    ls = [_log_softmax64(x[k].astype(np.float64)).astype(np.float32) for k in range(K)]
    with np.errstate(invalid="ignore"):
        g = ls[0] + np.float32(2.0) * (ls[0] - ls[1])
        g = g + np.float32(0.5) * (ls[0] - ls[2])
    fin = np.isfinite(want)
    for b in range(N - 1):
        assert np.abs(g[b][fin[b]].astype(np.float64) - want[b][fin[b]]).max() <= allow[b]
    wide = mg_ref.padded(x, mg_ref.aligned_ld(V), fill=1.0).reshape(K, N, -1)
    off = modality_guidance_scores(wide, (3.0, 1.5))[..., :V]
    for b in range(N - 1):
        assert np.abs(off[b][fin[b]] - want[b][fin[b]]).max() > allow[b]
    assert mg_ref.aligned_ld(256) == 264 and mg_ref.aligned_ld(257) == 264 and mg_ref.odd_ld(256) == 257 and mg_ref.odd_ld(257) == 259
