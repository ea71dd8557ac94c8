"""Min-p, locally typical, epsilon and eta sampling on the host: the float64 restatement (constraints.warp_filter) against the four
transformers warpers it restates, one at a time and chained; the range checks of the Python surface and of both C entries; the header,
the bindings and the exports; the search decoders' refusals.  No GPU: a bad argument fails before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.constraints import WARP_OFF, check_warp, warp_filter
from mmtg_amd.decode import BeamDecoder, ContrastiveDecoder

NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ 1. the restatement against transformers
def hf_chain(x, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """The kept set transformers' warpers leave of row x (float64 [V]), in generate's order."""
    from transformers.generation import logits_process as lp
    s = torch.from_numpy(np.asarray(x, dtype=np.float64))[None, :].clone()
    if min_p > 0.0:
        s = lp.MinPLogitsWarper(min_p=min_p)(None, s)
    if typical_p < 1.0:
        s = lp.TypicalLogitsWarper(mass=typical_p)(None, s)
    if epsilon_cutoff > 0.0:
        s = lp.EpsilonLogitsWarper(epsilon=epsilon_cutoff)(None, s)
    if eta_cutoff > 0.0:
        s = lp.EtaLogitsWarper(epsilon=eta_cutoff)(None, s)
    return (s[0] > -float("inf")).numpy()


def rows_for(seed, V=500):
    """Random rows of V ids (some with dropped ids, as a top-k / top-p filter or a ban leaves them), a tie at the cut, a one-hot row
    and a uniform row."""
    rng = np.random.default_rng(seed)
    rows = [rng.normal(size=V) * s for s in (1.0, 3.0, 6.0)]
    holes = rng.normal(size=V) * 3.0
    holes[rng.permutation(V)[:200]] = -np.inf
    tie = rng.normal(size=V) * 3.0
    order = np.argsort(-tie)
    tie[order[3:9]] = tie[order[3]]                       # six equal ids near the head: whichever cut lands there finds a tie
    tie[order[40:44]] = tie[order[40]]
    one_hot = np.full(V, -np.inf)
    one_hot[17] = 0.3
    near_one_hot = rng.normal(size=V)
    near_one_hot[5] += 30.0
    return rows + [holes, tie, one_hot, near_one_hot, np.zeros(V), np.full(V, -2.5)]


SETTINGS = ([dict(min_p=v) for v in (0.02, 0.1, 0.5, 1.0)] + [dict(typical_p=v) for v in (0.2, 0.5, 0.9, 0.95)]
            + [dict(epsilon_cutoff=v) for v in (3e-4, 3e-3, 0.05)] + [dict(eta_cutoff=v) for v in (3e-4, 2e-3, 0.05)]
            + [dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3), dict(typical_p=0.5, epsilon_cutoff=0.01),
               dict(min_p=0.1, eta_cutoff=0.02), dict(typical_p=0.2, eta_cutoff=0.05, epsilon_cutoff=0.02)])


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: ",".join("%s=%g" % i for i in kw.items()))
def test_the_restatement_keeps_what_the_transformers_warpers_keep(kw):
    seen = set()
    for seed in range(4):
        for i, x in enumerate(rows_for(seed)):
            got = warp_filter(x, **kw)
            kept = got > -np.inf
            assert np.array_equal(kept, hf_chain(x, **kw)), (seed, i, int(kept.sum()))
            assert np.array_equal(got[kept], x[kept]) and kept.any()              # values pass through; no stage empties a row
            seen.add(int(kept.sum()))
    assert len(seen) >= 2                                                        # the cut bites on some rows


def test_the_restatement_on_a_tie_a_one_hot_row_a_uniform_row_and_with_everything_off():
    V = 500
    uniform = np.zeros(V)
    assert (warp_filter(uniform, typical_p=0.3) > -np.inf).all()                 # every key ties: all stay
    assert (warp_filter(uniform, min_p=1.0, epsilon_cutoff=0.5, eta_cutoff=0.5) > -np.inf).all()     # everybody holds the maximum
    one_hot = np.full(V, -np.inf)
    one_hot[9] = 1.0
    for kw in SETTINGS:
        assert np.flatnonzero(warp_filter(one_hot, **kw) > -np.inf).tolist() == [9]
    x = np.random.default_rng(1).normal(size=V) * 3
    assert np.array_equal(warp_filter(x), x) and np.array_equal(warp_filter(x, *WARP_OFF), x)
    x[[3, 4, 5]] = x.max() + 1.0                                                 # a three-way tie at the maximum
    assert np.flatnonzero(warp_filter(x, min_p=1.0) > -np.inf).tolist() == [3, 4, 5]
    assert {3, 4, 5} <= set(np.flatnonzero(warp_filter(x, epsilon_cutoff=0.9) > -np.inf).tolist())
    two = warp_filter(np.stack([x, uniform]), typical_p=0.5)                     # rows are independent
    assert np.array_equal(two[0], warp_filter(x, typical_p=0.5)) and (two[1] > -np.inf).all()
    # typical sampling may drop the head: a flat bulk holds the entropy, the one likelier id is the atypical one
    head = np.zeros(V)
    head[0] = 3.0
    assert warp_filter(head, typical_p=0.5)[0] == -np.inf


def test_margins_report_the_distance_to_every_cut():
    x = np.random.default_rng(5).normal(size=500) * 3
    m = []
    warp_filter(x, min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3, margins=m)
    assert [(a, k) for a, k, _ in m] == [("min_p", "probability"), ("typical_p", "mass"), ("typical_p", "key"),
                                         ("epsilon_cutoff", "probability"), ("eta_cutoff", "probability")]
    assert all(d >= 0.0 for _, _, d in m)


# ------------------------------------------------------------------ 2. argument checks
BAD = [("min_p", -0.1), ("min_p", 1.5), ("min_p", float("nan")), ("typical_p", 0.0), ("typical_p", 1.01), ("typical_p", float("nan")),
       ("epsilon_cutoff", -1e-3), ("epsilon_cutoff", 1.0), ("eta_cutoff", 1.0), ("eta_cutoff", -0.5), ("eta_cutoff", float("nan"))]


@pytest.mark.parametrize("name,value", BAD)
def test_the_python_surface_names_the_argument_out_of_range(name, value):
    with pytest.raises(ValueError, match=name):
        check_warp(**{name: value})
    with pytest.raises(ValueError, match=name):
        warp_filter(np.zeros(8), **{name: value})
    with pytest.raises(ValueError, match=name):
        hip.logits_process_sample_warp(None, 8, 8, None, 1, None, 1.0, 1.0, 0, 0.0, None, None, 1, **{name: value})
    with pytest.raises(ValueError, match=name):
        hip.decode_sample_warp(None, 8, 8, torch.zeros(1, 8, dtype=torch.long), None, 0, 22, 1.0, 1.0, 0, 0.0,
                               tuple({**dict(zip(NAMES, WARP_OFF)), name: value}[k] for k in NAMES), None, 1, None)


def test_check_warp_takes_the_ends_of_the_ranges_and_refuses_what_is_no_number():
    assert check_warp() == WARP_OFF == (0.0, 1.0, 0.0, 0.0)
    assert check_warp(1, 1e-6, 0.999, np.float32(0.5)) == (1.0, 1e-6, 0.999, 0.5)
    for name in NAMES:
        for v in ("0.5", None, True):
            with pytest.raises(ValueError, match=name):
                check_warp(**{name: v})


def _c_args_process(uniforms=1, **kw):
    w = {**dict(zip(NAMES, WARP_OFF)), **kw}
    one = C.c_void_p(1)          # never dereferenced: the checks come before any device call
    return (one, 8, 8, one, 1, one, 1.0, 1.0, 0, 0.0, w["min_p"], w["typical_p"], w["epsilon_cutoff"], w["eta_cutoff"],
            C.c_void_p(uniforms), one, None, 1, None)


def _c_args_decode(uniforms=1, **kw):
    w = {**dict(zip(NAMES, WARP_OFF)), **kw}
    one = C.c_void_p(1)
    return (one, 8, 8, one, 64, one, 2, 22, 1.0, 1.0, 0, 0.0, w["min_p"], w["typical_p"], w["epsilon_cutoff"], w["eta_cutoff"],
            C.c_void_p(uniforms), 1, 1, None, None, 0, None, None, 3, None, 0, None, None, None, None, 0, one, None)


@pytest.mark.parametrize("entry,args", [("mmtg_logits_process_sample_warp", _c_args_process), ("mmtg_decode_sample_warp", _c_args_decode)])
def test_both_c_entries_return_minus_one_with_a_message_before_any_device_call(entry, args):
    L = hip.lib()
    f = getattr(L, entry)
    for name, value in BAD:
        assert f(*args(**{name: value})) == -1, (name, value)
        assert name in L.mmtg_last_error().decode(), (name, value)
    assert f(*args(uniforms=None)) == -1
    assert "uniforms" in L.mmtg_last_error().decode() or "bad args" in L.mmtg_last_error().decode()


def test_the_entries_are_declared_bound_and_exported_and_the_abi_version_is_12():
    header = open(os.path.join(HERE, "..", "include", "mmtg_hip.h")).read()
    for name in ("mmtg_logits_process_sample_warp", "mmtg_decode_sample_warp"):
        assert re.search(r"MMTG_API int %s\(" % name, header)
        assert name in hip.exported_symbols()
        assert getattr(hip.lib(), name).restype is C.c_int
    for word in NAMES:
        assert word in header
    assert "#define MMTG_ABI_VERSION 12" in header and hip.ABI_VERSION == 12 and hip.lib().mmtg_abi_version() == 12
    # the floats sit where the header puts them: after top_p, before uniforms
    sig = hip._SIGS["mmtg_decode_sample_warp"][0]
    assert sig[11:16] == [C.c_float] * 5 and len(sig) == len(hip._SIGS["mmtg_decode_sample_refrain"][0]) + 4
    sig = hip._SIGS["mmtg_logits_process_sample_warp"][0]
    assert sig[9:14] == [C.c_float] * 5 and len(sig) == len(hip._SIGS["mmtg_logits_process_sample"][0]) + 4


# ------------------------------------------------------------------ 3. refusals
@pytest.mark.parametrize("kw", [dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)])
def test_the_search_decoders_refuse_the_arguments_with_a_reason(kw):
    with pytest.raises(ValueError, match="search draws nothing"):
        BeamDecoder._refuse(**kw)
    with pytest.raises(ValueError, match="search draws nothing"):
        ContrastiveDecoder._refuse(**kw)
    BeamDecoder._refuse(**dict(zip(NAMES, WARP_OFF)))
    ContrastiveDecoder._refuse(**dict(zip(NAMES, WARP_OFF)))
    with pytest.raises(ValueError, match=next(iter(kw))):                        # out of range is said first, by name
        BeamDecoder._refuse(**{next(iter(kw)): 7.0})
