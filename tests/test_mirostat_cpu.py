"""Mirostat v2 on the host: the float64 restatement (constraints.mirostat_filter / mirostat_update) against an independent transcription
of the rule in llama.cpp's form; the control it exerts in simulation; its eta = 0 limit, the epsilon stage; the range checks of the
Python surface and of both C entries; the header, the bindings and the exports; the search decoders' refusals.  No GPU: a bad argument
fails before any device call."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from mmtg_amd import hip
from mmtg_amd.constraints import MIROSTAT_OFF, check_mirostat, mirostat_filter, mirostat_update, warp_filter
from mmtg_amd.decode import BeamDecoder, ContrastiveDecoder, GreedyDecoder
from test_warp_cpu import rows_for

HERE = os.path.dirname(os.path.abspath(__file__))
MUS = (0.5, 2.0, 4.0, 8.0, 40.0)


# ------------------------------------------------------------------ 1. the restatement against a transcription of llama.cpp's v2
def llama_v2(x, mu):
    """llama.cpp's mirostat v2 truncation of row x (float64 [V], -inf where dropped): sort descending, softmax, find the first sorted
    index whose surprise exceeds mu and truncate there (at least one stays), renormalise.  Returns (ids kept in sorted order, their
    renormalised probabilities)."""
    order = sorted((i for i in range(len(x)) if x[i] > -math.inf), key=lambda i: -x[i])      # (stable: ties in index order)
    top = x[order[0]]
    w = [math.exp(x[i] - top) for i in order]
    tot = math.fsum(w)
    p = [a / tot for a in w]
    cut = len(order)
    for k, pk in enumerate(p):
        if -math.log2(pk) > mu:
            cut = k
            break
    cut = max(cut, 1)
    tot = math.fsum(p[:cut])
    return order[:cut], [a / tot for a in p[:cut]]


def llama_update(ids, q, pick, mu, tau, eta):
    s = -math.log2(q[ids.index(pick)])
    return s, mu - eta * (s - tau)


def agrees_with_llama(x, mu, tau=2.0, eta=0.1):
    """The kept sets are equal but for the ids tied at the top, which the restatement all keeps where llama.cpp keeps the first; s and
    mu' agree to 1e-12 for every kept pick (where the sets are equal).  Returns the number kept."""
    got = mirostat_filter(x, mu)
    kept = np.flatnonzero(got > -np.inf).tolist()
    assert np.array_equal(got[kept], np.asarray(x, dtype=np.float64)[kept])       # values pass through
    ids, q = llama_v2(list(map(float, x)), mu)
    if sorted(ids) != kept:
        top = np.flatnonzero(x == np.max(x[np.asarray(x) > -np.inf])).tolist()
        assert len(ids) == 1 and len(top) > 1 and kept == top and ids[0] == top[0], (mu, ids, kept)
        return len(kept)
    for pick in kept:
        s, up = mirostat_update(got, pick, mu, tau, eta)
        s2, up2 = llama_update(ids, q, pick, mu, tau, eta)
        assert abs(s - s2) <= 1e-12 and abs(up - up2) <= 1e-12, (mu, pick, s, s2)
    return len(kept)


def test_the_restatement_is_llama_cpp_version_2_but_for_ties_at_the_top():
    sizes, tied = set(), 0
    for seed in range(4):
        for i, x in enumerate(rows_for(seed)):
            for mu in MUS:
                n = agrees_with_llama(x, mu)
                sizes.add(n)
                tied += i in (7, 8) and mu == 0.5           # the two flat rows: mu below every surprise, everybody holds the maximum
                if i in (7, 8) and mu == 0.5:
                    assert n == 500
    assert len(sizes) > 10 and tied == 8


def test_the_restatement_behind_typical_sampling_on_a_one_hot_row_and_below_zero():
    V = 500
    # behind typical_p the head may be gone: the survivors' maximum is what stays under a mu below every surprise
    head = np.zeros(V)
    head[0] = 3.0
    survivors = warp_filter(head, typical_p=0.5)
    assert survivors[0] == -np.inf and (survivors > -np.inf).sum() > 100
    assert np.array_equal(mirostat_filter(survivors, 0.5), survivors)            # they tie: all of them stay
    for seed in range(4):
        for x in rows_for(seed)[:5]:
            s = warp_filter(x, typical_p=0.5)
            for mu in MUS:
                agrees_with_llama(s, mu)
            low = mirostat_filter(s, 0.01)
            assert np.flatnonzero(low > -np.inf).tolist() == np.flatnonzero(s == s.max()).tolist()
    # a one-hot row: s = 0, and mu rises by eta * tau
    one_hot = np.full(V, -np.inf)
    one_hot[17] = 0.3
    for mu in MUS + (-3.0,):
        f = mirostat_filter(one_hot, mu)
        assert np.flatnonzero(f > -np.inf).tolist() == [17]
        s, up = mirostat_update(f, 17, mu, 3.0, 0.25)
        assert s == 0.0 and up == mu + 0.25 * 3.0
    # mu < 0: no surprise is below it; the maximum alone stays, s = 0
    x = np.random.default_rng(0).normal(size=V) * 3
    f = mirostat_filter(x, -1.0)
    assert np.flatnonzero(f > -np.inf).tolist() == [int(np.argmax(x))]
    assert mirostat_update(f, int(np.argmax(x)), -1.0, 2.0, 0.1) == (0.0, -1.0 + 0.2)
    agrees_with_llama(x, -1.0)
    with pytest.raises(ValueError, match="kept"):
        mirostat_update(f, int(np.argmin(x)), -1.0, 2.0, 0.1)
    m = []
    mirostat_filter(one_hot, 2.0, margins=m)
    assert m == [("mirostat_tau", "surprise", 2.0)]
    m = []
    mirostat_filter(x, 4.0, margins=m)
    assert len(m) == V and all(a == "mirostat_tau" and k == "surprise" and d >= 0.0 for a, k, d in m)


# ------------------------------------------------------------------ 2. the control
def simulate(tau, eta, scale, rows=32, steps=300, V=500, late_from=100):
    """rows independent chains of `steps` draws on fresh rows `normal * scale`: per row the mean surprise over steps 100 and later, the
    final mu, and whether every survivor was kept on each step from late_from on."""
    means, mus, full = [], [], []
    for r in range(rows):
        rng = np.random.default_rng(1000 * r + 7)
        mu, late, all_kept = 2.0 * tau, [], True
        for t in range(steps):
            x = rng.normal(size=V) * scale
            f = mirostat_filter(x, mu)
            q = np.exp(f - f.max())
            cdf = np.cumsum(q)
            pick = min(int(np.searchsorted(cdf, rng.random() * cdf[-1], side="right")), V - 1)
            s, mu = mirostat_update(f, pick, mu, tau, eta)
            if t >= 100:
                late.append(s)
            if t >= late_from:
                all_kept &= bool((f > -np.inf).all())
        means.append(float(np.mean(late)))
        mus.append(mu)
        full.append(all_kept)
    return np.array(means), np.array(mus), full


@pytest.mark.parametrize("tau", [1.0, 2.0, 3.0])
def test_the_mean_surprise_settles_at_tau(tau):
    means, _, _ = simulate(tau, 0.1, 2.0)
    print("tau %g: mean surprise over steps 100.. in [%.4f, %.4f], worst distance %.4f" % (tau, means.min(), means.max(), np.abs(means - tau).max()))
    assert np.abs(means - tau).max() <= 0.15
    if tau == 2.0:      # what the control is for: untruncated draws on such rows carry more than 5 bits
        rng = np.random.default_rng(3)
        plain = []
        for _ in range(300):
            x = rng.normal(size=500) * 2.0
            p = np.exp(x - x.max())
            p /= p.sum()
            plain.append(-math.log2(p[rng.choice(500, p=p)]))
        assert np.mean(plain) > 5.0


def test_a_target_out_of_reach_opens_the_cut_entirely():
    """tau = 5 on normal * 3 rows: untruncated draws carry about 4.3 bits, so no cut reaches 5: mu grows, the late steps keep every
    survivor, and the mean surprise stays below tau.  Which steps are late follows from the rule: mu climbs from 10 by eta * (tau - s),
    and a row's mean s is at most about 4.55 bits here, so by 0.045 bits a step or more; the rarest of 500 such ids has a surprise of up
    to about 33 bits (its logit some 20 nats under the largest), so the cut is fully open after at most some 500 steps.  The chains
    run 900 steps and the last 100 are the late ones."""
    means, mus, full = simulate(5.0, 0.1, 3.0, steps=900, late_from=800)
    print("mean surprise in [%.3f, %.3f], final mu in [%.2f, %.2f]" % (means.min(), means.max(), mus.min(), mus.max()))
    assert all(full) and (mus > 2 * 5.0).all() and (means < 5.0).all()


# ------------------------------------------------------------------ 3. eta = 0 is the epsilon stage
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0, 3.0, 5.0])
def test_a_frozen_mu_is_epsilon_sampling_at_two_to_the_minus_two_tau(tau):
    differ = 0
    for seed in range(4):
        for x in rows_for(seed):
            got, want = mirostat_filter(x, 2 * tau), warp_filter(x, epsilon_cutoff=2.0 ** (-2 * tau))
            assert np.array_equal(got, want), seed
            differ += int((got > -np.inf).sum() < (x > -np.inf).sum())
            f = mirostat_filter(x, 2 * tau)
            assert mirostat_update(f, int(np.argmax(x)), 2 * tau, tau, 0.0)[1] == 2 * tau          # eta = 0 freezes mu
    assert differ >= 8


# ------------------------------------------------------------------ 4. argument checks
BAD = [("mirostat_tau", -1.0), ("mirostat_tau", 32.5), ("mirostat_tau", float("nan")), ("mirostat_tau", float("inf")),
       ("mirostat_eta", -0.1), ("mirostat_eta", 1.5), ("mirostat_eta", float("nan"))]


@pytest.mark.parametrize("name,value", BAD)
def test_the_python_surface_names_the_argument_out_of_range(name, value):
    base = {"mirostat_tau": 2.0, "mirostat_eta": 0.1}
    with pytest.raises(ValueError, match=name):
        check_mirostat(**{**base, name: value})
    a = {**base, name: value}
    with pytest.raises(ValueError, match=name):
        hip.logits_process_sample_mirostat(None, 8, 8, None, 1, None, 1.0, 1.0, 0, 0.0, None, None, 1, a["mirostat_tau"], a["mirostat_eta"],
                                           None)
    with pytest.raises(ValueError, match=name):
        hip.decode_sample_mirostat(None, 8, 8, torch.zeros(1, 8, dtype=torch.long), None, 0, 22, 1.0, 1.0, 0, 0.0, (0.0, 1.0, 0.0, 0.0),
                                   (a["mirostat_tau"], a["mirostat_eta"]), None, None, 1, None)
    with pytest.raises(ValueError, match=name):
        GreedyDecoder.begin(None, None, 8, **a)                                  # the first thing begin looks at after keywords
    with pytest.raises(ValueError, match=name):
        BeamDecoder._refuse(**a)


def test_check_mirostat_takes_the_ends_of_the_ranges_and_refuses_what_is_no_number():
    assert check_mirostat() == MIROSTAT_OFF == (0.0, 0.1)
    assert check_mirostat(32, 1) == (32.0, 1.0) and check_mirostat(np.float32(0.5), 0) == (0.5, 0.0)
    for name in ("mirostat_tau", "mirostat_eta"):
        for v in ("0.5", None, True):
            with pytest.raises(ValueError, match=name):
                check_mirostat(**{name: v})
    for wrapper in ("logits_process_sample_mirostat", "decode_sample_mirostat"):   # 0 is "off", which these entries do not have
        with pytest.raises(ValueError, match="mirostat_tau"):
            if wrapper == "decode_sample_mirostat":
                hip.decode_sample_mirostat(None, 8, 8, torch.zeros(1, 8, dtype=torch.long), None, 0, 22, 1.0, 1.0, 0, 0.0,
                                           (0.0, 1.0, 0.0, 0.0), (0.0, 0.1), None, None, 1, None)
            else:
                hip.logits_process_sample_mirostat(None, 8, 8, None, 1, None, 1.0, 1.0, 0, 0.0, None, None, 1, 0.0, 0.1, None)


def _c_args_process(tau=2.0, eta=0.1, mu=1, min_p=0.0):
    one = C.c_void_p(1)          # never dereferenced: the checks come before any device call
    return (one, 8, 8, one, 1, one, 1.0, 1.0, 0, 0.0, min_p, 1.0, 0.0, 0.0, one, one, None, 1, tau, eta, C.c_void_p(mu), None, None)


def _c_args_decode(tau=2.0, eta=0.1, mu=1, min_p=0.0):
    one = C.c_void_p(1)
    return (one, 8, 8, one, 64, one, 2, 22, 1.0, 1.0, 0, 0.0, min_p, 1.0, 0.0, 0.0, one, 1, 1, None, None, 0, None, None, 3, None, 0, None,
            None, None, None, 0, one, tau, eta, C.c_void_p(mu), None)


@pytest.mark.parametrize("entry,args", [("mmtg_logits_process_sample_mirostat", _c_args_process),
                                        ("mmtg_decode_sample_mirostat", _c_args_decode)])
def test_both_c_entries_return_minus_one_with_a_message_before_any_device_call(entry, args):
    L = hip.lib()
    f = getattr(L, entry)
    for name, value in BAD + [("mirostat_tau", 0.0)]:
        kw = {"tau" if name == "mirostat_tau" else "eta": value}
        assert f(*args(**kw)) == -1, (name, value)
        assert name in L.mmtg_last_error().decode(), (name, value)
    assert f(*args(mu=None)) == -1                                               # a null mu is refused
    assert "mu" in L.mmtg_last_error().decode()
    assert f(*args(min_p=1.5)) == -1                                             # the four cuts keep their checks
    assert "min_p" in L.mmtg_last_error().decode()


def test_the_entries_are_declared_bound_and_exported_and_the_abi_version_is_12():
    header = open(os.path.join(HERE, "..", "include", "mmtg_hip.h")).read()
    for name in ("mmtg_logits_process_sample_mirostat", "mmtg_decode_sample_mirostat"):
        assert re.search(r"MMTG_API int %s\(" % name, header)
        assert name in hip.exported_symbols()
        assert getattr(hip.lib(), name).restype is C.c_int
    for word in ("mirostat_tau", "mirostat_eta", "llama.cpp keeps only the first id"):
        assert word in header
    assert "#define MMTG_ABI_VERSION 12" in header and hip.ABI_VERSION == 12 and hip.lib().mmtg_abi_version() == 12
    # the warp entries' arguments, then tau, eta, mu (and surprise) before the stream
    warp, miro = hip._SIGS["mmtg_decode_sample_warp"][0], hip._SIGS["mmtg_decode_sample_mirostat"][0]
    assert miro[:len(warp) - 1] == warp[:-1] and miro[len(warp) - 1:] == [C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    warp, miro = hip._SIGS["mmtg_logits_process_sample_warp"][0], hip._SIGS["mmtg_logits_process_sample_mirostat"][0]
    assert miro[:len(warp) - 1] == warp[:-1] and miro[len(warp) - 1:] == [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    assert callable(hip.logits_process_sample_mirostat) and callable(hip.decode_sample_mirostat)


# ------------------------------------------------------------------ 5. refusals
def test_the_search_decoders_refuse_the_arguments_with_a_reason():
    for kw in (dict(mirostat_tau=2.0), dict(mirostat_tau=0.5, mirostat_eta=0.0)):
        with pytest.raises(ValueError, match="search draws nothing"):
            BeamDecoder._refuse(**kw)
        with pytest.raises(ValueError, match="search draws nothing"):
            ContrastiveDecoder._refuse(**kw)
    BeamDecoder._refuse(mirostat_tau=MIROSTAT_OFF[0], mirostat_eta=MIROSTAT_OFF[1])
    BeamDecoder._refuse(mirostat_tau=0.0, mirostat_eta=0.5)                                           # eta alone turns nothing on
    ContrastiveDecoder._refuse(mirostat_tau=0.0, mirostat_eta=0.1)
    with pytest.raises(ValueError, match="mirostat_tau"):                        # out of range is said first, by name
        ContrastiveDecoder._refuse(mirostat_tau=77.0)
    for cls in (BeamDecoder, ContrastiveDecoder):                                # begin and generate take the names, and refuse them
        assert {"mirostat_tau", "mirostat_eta"} <= {k for names, _, _ in cls._REFUSED for k in names}
        for fn in (cls.begin, cls.generate):
            with pytest.raises(ValueError, match="search draws nothing"):
                fn(None, {}, 8, mirostat_tau=2.0, mirostat_eta=0.1)
