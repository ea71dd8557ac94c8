"""Stochastic beam search (mmtg_amd.decode.StochasticBeamDecoder): the host side of its two ABI entries, the host checks, the
float64 restatements of the rule (constraints.gumbel_candidates / gumbel_merge) and the CPU search that pins the decoder.

The reference (src/generate.py) draws its samples independently, so no golden file can pin the feature.  What pins it: the
restatements' own algebra and distribution (the noise is a hash, so nothing random is left: the chi-square test below is a fixed
computation), and `cpu_stochastic_beam_search`, which runs the restatements on the committed oracle (CachedForward,
process_logits, the cadence and sticky PAD of tests/test_beam_cpu.py's cpu_beam_search).  tests/test_stochastic_gpu.py holds the
kernels and the decoder to them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_lines_cpu as L
from mmtg_amd import hip
from mmtg_amd.constraints import (check_lines, check_stochastic, gumbel_candidates, gumbel_merge, gumbel_noise, gumbel_uniforms,
                                  stochastic_row_seeds)
from mmtg_amd.decode import StochasticBeamDecoder
from oracle import mmtg_oracle as O
from test_beam_cpu import SENT, _fork, comparable_length, setup_case, start_row
from test_ngram_cpu import banned_ids
from test_prefix_cpu import _base
from test_template_cpu import fixture_templates, template_violations

T, REP = 1.1, 1.5
NB, LENGTH, SEED = 4, 120, 11        # what tests/test_stochastic_gpu.py follows the CPU search at
CASES = ("tiny_s5", "tiny_lstm2_rnn2")


# ------------------------------------------------------------------ the entries and the host checks
def test_gumbel_entry_points_are_declared_bound_exported_and_reject_bad_arguments_without_a_gpu():
    """The two new ABI entries are in the header, in hip._SIGS and in the library, the ABI version is still 12, and bad arguments
    return -1 with a message that names the argument, before any device call."""
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmtg_hip.h")).read()
    lib = ctypes.CDLL(hip.lib_path())
    for name in ("mmtg_decode_gumbel_candidates", "mmtg_decode_gumbel_merge"):
        assert name + "(" in header and name in hip.exported_symbols() and hasattr(lib, name)
    assert callable(hip.decode_gumbel_candidates) and callable(hip.decode_gumbel_merge)
    Lb = hip.lib()
    assert Lb.mmtg_abi_version() == hip.ABI_VERSION == 12
    p = [0x7000000000 + (i << 24) for i in range(16)]

    def cand(nb=4, scores=p[6], gum=p[7], row_seed=p[8], cand_g=p[9], src=p[5], n_lines=11):
        return Lb.mmtg_decode_gumbel_candidates(p[0], 160, 160, p[1], 256, p[2], 5, SENT, 1.1, 1.5, nb, p[3], p[4], 8, None, 0, None, None,
                                                n_lines, None, 0, None, None, None, None, 0, src, scores, gum, row_seed, cand_g, None)

    for nb in (0, 17):
        assert cand(nb=nb) == -1 and b"decode_gumbel_candidates: nb = %d" % nb in Lb.mmtg_last_error()
    for arg in ("scores", "gum", "row_seed", "cand_g"):
        assert cand(**{arg: None}) == -1 and b"decode_gumbel_candidates: " + arg.encode() in Lb.mmtg_last_error()
    assert cand(src=None) == -1 and b"decode_gumbel_candidates: src" in Lb.mmtg_last_error()

    def merge(nb=4, gum=p[4], cand_g=p[2], pos_next=p[10], scores=p[3]):
        return Lb.mmtg_decode_gumbel_merge(p[0], p[1], cand_g, scores, gum, p[5], 256, p[6], 256, p[7], 256, p[8], 5, SENT, nb, 2, pos_next,
                                           None, None)

    for nb in (0, 17):
        assert merge(nb=nb) == -1 and b"decode_gumbel_merge: nb = %d" % nb in Lb.mmtg_last_error()
    assert merge(gum=None) == -1 and b"decode_gumbel_merge: gum" in Lb.mmtg_last_error()
    assert merge(cand_g=None) == -1 and b"decode_gumbel_merge: cand_g" in Lb.mmtg_last_error()
    assert merge(pos_next=p[8]) == -1 and b"decode_gumbel_merge: pos_next must not alias pos_ptr" in Lb.mmtg_last_error()
    assert merge(scores=None) == -1 and b"decode_gumbel_merge: null pointer" in Lb.mmtg_last_error()


def test_stochastic_host_checks_raise_before_device_work():
    assert check_stochastic(4, 0) == (4, 0) and check_stochastic(np.int64(16), 2 ** 32 - 1) == (16, 2 ** 32 - 1)
    for nb in (0, 17, -1):
        with pytest.raises(ValueError, match="num_samples"):
            check_stochastic(nb)
    for nb in (2.0, "4", True, None):
        with pytest.raises(ValueError, match="num_samples must be an integer"):
            check_stochastic(nb)
    for seed in (-1, 2 ** 32, 1.5, "7", None):
        with pytest.raises(ValueError, match="seed"):
            check_stochastic(4, seed)
    for nb in (0, 17):
        with pytest.raises(ValueError, match="num_samples"):
            StochasticBeamDecoder(None, 2, nb)
    with pytest.raises(ValueError, match="one lane"):
        StochasticBeamDecoder(None, 2, 4, lanes=2)
    refusals = ((dict(keywords=[(5, 6)]), "no keywords=.*draw order"), (dict(num_beam_groups=2), "num_beam_groups.*distribution"),
                (dict(diversity_penalty=1.0), "diversity_penalty.*distribution"), (dict(return_logprobs=True), "return_logprobs.*score_sequences"),
                (dict(top_k=10), "no sampling top_k"), (dict(top_p=0.7), "no sampling top_k / top_p"), (dict(generator=object()), "generator"),
                (dict(min_p=0.1), "truncate"), (dict(typical_p=0.9), "truncate"), (dict(epsilon_cutoff=0.01), "truncate"),
                (dict(eta_cutoff=0.01), "truncate"), (dict(mirostat_tau=2.0), "mirostat"))
    from mmtg_amd.generate import generate_stochastic_beams
    for kw, match in refusals:
        with pytest.raises(ValueError, match=match):
            StochasticBeamDecoder._refuse(**kw)
        with pytest.raises(ValueError, match=match):
            StochasticBeamDecoder.begin(None, {}, 8, **kw)
        with pytest.raises(ValueError, match=match):
            StochasticBeamDecoder.generate(None, {}, 8, **kw)
        with pytest.raises(ValueError, match=match):
            generate_stochastic_beams(None, [], None, **kw)
    StochasticBeamDecoder._refuse()
    with pytest.raises(ValueError, match="num_samples"):
        generate_stochastic_beams(None, [], None, num_samples=17)
    with pytest.raises(ValueError, match="seed"):
        generate_stochastic_beams(None, [], None, seed=-3)


def test_row_seeds_do_not_depend_on_the_chunking():
    whole = stochastic_row_seeds(7, 0, 10, 4)
    assert whole.dtype == np.uint32 and whole.shape == (40,) and len(set(whole.tolist())) == 40
    for per in (1, 3, 4, 10):
        parts = [stochastic_row_seeds(7, lo, min(per, 10 - lo), 4) for lo in range(0, 10, per)]
        assert np.array_equal(np.concatenate(parts), whole)
    # a prompt's words do not depend on nb's other slots, and another seed gives other words
    assert np.array_equal(stochastic_row_seeds(7, 3, 1, 2), whole[12:14])
    assert not np.intersect1d(stochastic_row_seeds(8, 0, 10, 4), whole).size
    assert stochastic_row_seeds(0, 0, 1, 1)[0] != 0


def test_the_noise_is_the_hash_of_the_header():
    """gumbel_uniforms against a plain-Python murmur3 finaliser, and u strictly inside (0, 1) on the fp32 grid the header states."""
    def h32(seed, idx):
        h = (idx * 0x9E3779B1 + seed) & 0xFFFFFFFF
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)

    words = np.array([0, 1, 0xFFFFFFFF, 123456789], np.uint32)
    u = gumbel_uniforms(words, 37, 300)
    assert u.dtype == np.float32 and u.shape == (4, 300)
    for b, wd in enumerate(words.tolist()):
        for v in (0, 1, 5, 299):
            assert float(u[b, v]) == ((h32(h32(wd, 37), v) >> 9) + 0.5) * 2.0 ** -23
    assert (u > 0).all() and (u < 1).all()
    n = gumbel_noise(words, 37, 300)
    assert n.dtype == np.float64 and np.isfinite(n).all() and not np.array_equal(n, gumbel_noise(words, 38, 300))


# ------------------------------------------------------------------ the restatements alone
def _random_rows(R, V, rng):
    x = rng.normal(0.0, 2.0, (R, V))
    x[:, [1, 2, 100, 102][:sum(v < V for v in (1, 2, 100, 102))]] = -np.inf
    x[rng.random((R, V)) < 0.1] = -np.inf
    scores = -rng.random(R) * 40.0
    gum = -rng.random(R) * 5.0
    return x, scores, gum


def test_restatement_algebra_over_random_rows():
    """gumbel_candidates in float64 over 600 random rows: slot 0 passes the parent's value on exactly, cand_g does not increase in
    rank and never exceeds the parent's, cand_val is the log-softmax of the offered id, the ids are distinct and allowed; a dead
    row and an all-banned row offer -inf and no NaN; a single-choice column passes the parent's value on."""
    rng = np.random.default_rng(5)
    R, V = 600, 128
    x, scores, gum = _random_rows(R, V, rng)
    gum[::7] = 0.0
    dead, banned = [3, 50], [4, 51]
    gum[dead[0]], scores[dead[1]] = -np.inf, -np.inf
    x[banned] = -np.inf
    only = np.full(R, -1)
    only[[10, 11, 3]] = [0, 77, 5]                                 # (row 3 is dead: dead wins)
    words = stochastic_row_seeds(1, 0, R, 1)
    for nb in (1, 4, 16):
        gaps = []
        ids, val, g = gumbel_candidates(x, scores, gum, words, 40, nb, only=only, gaps=gaps)
        assert not np.isnan(val).any() and not np.isnan(g).any() and len(gaps) == R
        for b in dead + banned:
            assert (ids[b] == 0).all() and np.isneginf(val[b]).all() and np.isneginf(g[b]).all()
        for b, v in ((10, 0), (11, 77)):
            assert ids[b, 0] == v and val[b, 0] == 0.0 and g[b, 0] == gum[b]
            assert (ids[b, 1:] == 0).all() and np.isneginf(val[b, 1:]).all() and np.isneginf(g[b, 1:]).all()
        for b in range(R):
            if b in dead + banned + [10, 11]:
                continue
            assert g[b, 0] == gum[b]                                # bit for bit
            assert (np.diff(g[b]) <= 0).all() and (g[b] <= gum[b]).all()
            assert len(set(ids[b].tolist())) == nb and np.isfinite(x[b, ids[b]]).all()
            ok = np.isfinite(x[b])
            lse = np.log(np.exp(x[b, ok] - x[b, ok].max()).sum()) + x[b, ok].max()
            assert np.allclose(val[b], x[b, ids[b]] - lse, rtol=0, atol=1e-12)
            t = val[b] + gumbel_noise(words[b:b + 1], 40, V)[0, ids[b]]
            assert (np.diff(t) <= 0).all()
            if nb < ok.sum():
                rest = np.setdiff1d(np.flatnonzero(ok), ids[b])
                tr = (x[b, rest] - lse) + gumbel_noise(words[b:b + 1], 40, V)[0, rest]
                assert np.isclose(gaps[b], t[-1] - tr.max(), rtol=0, atol=1e-12) and gaps[b] >= 0


def test_merge_restatement_on_hand_written_candidates():
    nb, P, pos = 2, 3, 7                                            # j = 5: a free column
    seq = np.arange(2 * nb * 40, dtype=np.int64).reshape(2 * nb, 40) + 200
    keep, rows = np.ones((2 * nb, 40), np.int32), np.tile(np.arange(2 * nb, dtype=np.int32)[:, None], (1, 40))
    scores, gum = np.array([-1.0, -2.0, -3.0, -np.inf], np.float32), np.array([0.0, -0.5, 0.0, -np.inf], np.float32)
    cv = np.array([[-0.5, -1.5], [-0.25, -2.0], [-1.0, -np.inf], [-np.inf, -np.inf]], np.float32)
    ci = np.array([[30, 31], [32, 33], [34, 0], [0, 0]], np.int32)
    cg = np.array([[0.0, -0.7], [-0.5, -0.5], [0.0, np.nan], [-np.inf, -np.inf]], np.float32)
    old = seq.copy()
    gaps = []
    par = gumbel_merge(cv, ci, cg, scores, gum, seq, keep, rows, pos, P, SENT, nb, gaps=gaps)
    assert par.tolist() == [0, 1, 2, 2]                             # prompt 0: (p0, r0) then the tie -0.5 by parent 1 rank 0
    assert seq[:, pos + 1].tolist() == [30, 32, 34, 0] and np.array_equal(seq[:, :pos + 1], old[par, :pos + 1])
    assert np.array_equal(seq[:, pos + 2:], old[:, pos + 2:]) and rows[:, pos + 1].tolist() == [0, 1, 2, 3]
    assert scores.tolist() == [-1.5, -2.25, -4.0, -np.inf] and gum.tolist() == [0.0, -0.5, 0.0, -np.inf]
    assert gaps[0] == 0.0 and gaps[1] == float("inf")
    # a forced column and null candidates: identity, gum untouched
    g0 = gum.copy()
    gumbel_merge(cv, ci, cg, scores, gum, seq, keep, rows, P + SENT - 2, P, SENT, nb)
    assert (seq[:, P + SENT - 1] == 2).all() and np.array_equal(gum, g0)
    gumbel_merge(None, None, None, scores, gum, seq, keep, rows, pos, P, SENT, nb)
    assert np.array_equal(gum, g0) and seq[:, pos + 1].tolist() == [30, 32, 34, 0]


def test_the_restatement_samples_without_replacement_from_the_softmax():
    """One row of logits over V = 128 with six ids holding most of the mass (ids 1, 2, 100, 102 excluded, as the kernels exclude them),
    8192 row seeds from seed 0, nb = 2: the first offers against the softmax, and the ordered pairs against p_i p_j / (1 - p_i),
    pass a chi-square test at the 99.9 % quantile (cells with an expectation below 5 pooled)."""
    from scipy.stats import chi2
    V, N, nb = 128, 8192, 2
    x = np.random.default_rng(0).normal(0.0, 0.5, V)
    x[[7, 20, 33, 64, 101, 127]] += np.array([5.0, 4.6, 4.3, 4.0, 3.8, 3.5])
    x[[1, 2, 100, 102]] = -np.inf
    p = np.exp(x - x[np.isfinite(x)].max())
    p[~np.isfinite(x)] = 0.0
    p /= p.sum()
    assert np.sort(p)[-6:].sum() > 0.7
    words = stochastic_row_seeds(0, 0, N, 1)
    ids, val, g = gumbel_candidates(np.tile(x, (N, 1)), np.zeros(N), np.zeros(N), words, 17, nb)
    assert (g[:, 0] == 0.0).all() and (ids[:, 0] != ids[:, 1]).all() and not np.isin(ids, [1, 2, 100, 102]).any()

    def chi_square(counts, expect):
        big = expect >= 5.0
        obs, exp_ = np.append(counts[big], counts[~big].sum()), np.append(expect[big], expect[~big].sum())
        if exp_[-1] == 0:
            obs, exp_ = obs[:-1], exp_[:-1]
        stat, df = float(((obs - exp_) ** 2 / exp_).sum()), len(exp_) - 1
        print("chi-square %.1f at %d degrees of freedom (99.9 %% quantile %.1f)" % (stat, df, chi2.ppf(0.999, df)))
        return stat, chi2.ppf(0.999, df)

    stat, q = chi_square(np.bincount(ids[:, 0], minlength=V).astype(float), N * p)
    assert stat < q
    pair = np.zeros((V, V))
    np.add.at(pair, (ids[:, 0], ids[:, 1]), 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        expect = N * p[:, None] * p[None, :] / (1.0 - p[:, None])
    expect[np.arange(V), np.arange(V)] = 0.0
    expect[~np.isfinite(expect)] = 0.0
    assert abs(expect.sum() - N) < 1e-6
    stat, q = chi_square(pair.reshape(-1), expect.reshape(-1))
    assert stat < q


# ------------------------------------------------------------------ the CPU search on the oracle
def _column(cf, base, ids, c, V, tables, b, n):
    """(x, only) of lyric column c for a row whose history is ids: the processed logits under every rule (float64, -inf where banned),
    or the one id a single-choice column holds (sticky PAD, a full line's PAD, a template's given id)."""
    logits = cf(dict(base, targets=torch.tensor([ids], dtype=torch.long)))[0, -1, :]
    if ids[-1] == 0:
        return None, 0
    x = O.process_logits(logits, torch.tensor(ids), T, REP)[:V].clone()
    for v in banned_ids(ids, n):
        x[v] = float("-inf")
    if tables is not None:
        lo, hi, ends = tables.bounds(b, c // SENT)
        if L.line_rule(ids, lo, hi, ends) == "pad":
            return None, 0
        y = tables.symbol(b, c // SENT, c % SENT - 1) if tables.tmpl is not None else None
        if isinstance(y, int):
            return None, y
        if y is not None:
            keep = torch.zeros_like(x, dtype=torch.bool)
            keep[sorted(y)] = True
            keep[0] = True
            x[~keep] = float("-inf")
        x = L.apply_rule(x, ids, lo, hi, ends)
    return x.double().numpy(), -1


def cpu_stochastic_beam_search(w, sh, table, start, length, nb, words, tables=None, b=0, n=0, prefix=(1,)):
    """One prompt (`start`: a dataset row without targets), nb rows whose seed words are `words`: the restatements
    constraints.gumbel_candidates / gumbel_merge on the oracle's processed logits, with the cadence of cpu_beam_search.  The state is
    kept as the decoder keeps it (fp32 scores and gum; the noise of lyric column c is drawn at position P + c - 1).  Returns (ids [nb,
    1 + length] in draw order, scores [nb] fp32, gum [nb] fp32, gaps): gaps[i] = (the lyric column, the smallest gap that decided
    anything there: between the nb-th and (nb + 1)-th t of a live parent, or the nb-th and (nb + 1)-th cand_g of the merge)."""
    base = _base(start)
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    p = [int(v) for v in prefix]
    seq = np.zeros((nb, length + 2), np.int64)
    seq[:, :len(p)] = p
    keep, rows = np.ones_like(seq, dtype=np.int32), np.tile(np.arange(nb, dtype=np.int32)[:, None], (1, length + 2))
    scores = np.full(nb, -np.inf, np.float32)
    scores[0] = 0.0
    gum = scores.copy()
    cfs = [O.CachedForward(w, sh, table)]
    cfs += [_fork(cfs[0]) for _ in range(nb - 1)]
    gaps = []
    with torch.no_grad():
        for c in range(len(p), length + 1):
            pos = c - 1                                             # (P = 0 in the merge's layout: j = pos + 1 = c)
            if c % SENT in (0, SENT - 1):
                gumbel_merge(None, None, None, scores, gum, seq, keep, rows, pos, 0, SENT, nb)
                continue
            x, only = np.full((nb, V), -np.inf), np.full(nb, -1)
            for r in range(nb):
                if gum[r] > -np.inf:
                    xr, only[r] = _column(cfs[r], base, seq[r, :c].tolist(), c, V, tables, b, n)
                    if xr is not None:
                        x[r] = xr
            cgaps = []
            ci, cv, cg = gumbel_candidates(x, scores, gum, words, sh.P + c - 1, nb, only=only, gaps=cgaps)
            par = gumbel_merge(cv.astype(np.float32), ci.astype(np.int32), cg.astype(np.float32), scores, gum, seq, keep, rows, pos, 0,
                               SENT, nb, gaps=cgaps)
            gaps.append((c, min(cgaps)))
            cfs = [_fork(cfs[q]) for q in par.tolist()]
    return seq[:, :length + 1].copy(), scores, gum, gaps


def teacher_forced_score(w, sh, table, start, ids, tables=None, b=0, n=0):
    """The sum of the processed log-probabilities (fp32 log_softmax under every rule) of a row's model-chosen columns."""
    base = _base(start)
    V = min(int(w["decoder.gpt2.lm_head.weight"].shape[0]), 13317)
    cf, total = O.CachedForward(w, sh, table), 0.0
    ids = [int(v) for v in ids]
    with torch.no_grad():
        for c in range(1, len(ids)):
            if c % SENT in (0, SENT - 1):
                continue
            x, only = _column(cf, base, ids[:c], c, V, tables, b, n)
            if x is None:
                assert ids[c] == only
                continue
            total += float(torch.log_softmax(torch.from_numpy(x).float(), -1)[ids[c]])
    return total


@functools.lru_cache(maxsize=None)
def follow_runs(case):
    """The CPU search of every prompt of fixture `case` at (NB, LENGTH, SEED), run once and shared (the GPU tests read it too)."""
    fx, sh, w, table, batch = setup_case(case)
    n = batch["topic_ids"].shape[0]
    words = stochastic_row_seeds(SEED, 0, n, NB).reshape(n, NB)
    return [cpu_stochastic_beam_search(w, sh, table, start_row(batch, row), LENGTH, NB, words[row]) for row in range(n)]


@pytest.mark.parametrize("case", CASES)
def test_cpu_stochastic_beam_search_rules_and_comparable_length(case):
    """Four rows, 120 steps: the forced cadence on every row, pairwise different rows, gum[0] == 0 and non-increasing, scores equal
    to the teacher-forced sums of processed log-probabilities -- and the smallest deciding gap per step, which gives the length up
    to which tests/test_stochastic_gpu.py may hold an fp32 search to this one."""
    fx, sh, w, table, batch = setup_case(case)
    lens = []
    for row, (ids, scores, gum, gaps) in enumerate(follow_runs(case)):
        assert ids.shape == (NB, 1 + LENGTH) and (ids[:, 0] == 1).all()
        assert np.isfinite(scores).all() and np.isfinite(gum).all() and gum[0] == 0.0 and (np.diff(gum) <= 0).all()
        assert len({tuple(r) for r in ids.tolist()}) == NB
        for j in range(2, 1 + LENGTH):
            if (j + 1) % SENT == 0:
                assert (ids[:, j] == 2).all()
            elif (j + 1) % SENT == 1:
                assert (ids[:, j] == 1).all()
            else:
                assert not np.isin(ids[:, j], [1, 2, 100, 102]).any()
        for r in range(NB):
            # (about a hundred fp32 additions at magnitudes up to |score|, each within 2^-24 |score|, and as many fp32 log-probabilities)
            assert abs(teacher_forced_score(w, sh, table, start_row(batch, row), ids[r]) - float(scores[r])) < 1e-3 + 2e-5 * abs(float(scores[r]))
        assert len(gaps) == sum(1 for c in range(1, LENGTH + 1) if c % SENT not in (0, SENT - 1)) and all(g >= 0 for _, g in gaps)
        lens.append(comparable_length(gaps, LENGTH))
    print(case, "comparable lengths", lens)
    assert max(lens) >= 60, lens


def test_cpu_stochastic_beam_search_obeys_line_lengths_and_an_acrostic():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    kw, _, _, _ = fixture_templates(fx)
    acro = kw["templates"][0]
    length = 6 * SENT
    t = check_lines(7, None, 1, length, SENT, 160, templates=acro)
    words = stochastic_row_seeds(SEED, 0, 1, NB)
    ids, scores, gum, _ = cpu_stochastic_beam_search(w, sh, table, start_row(batch, 0), length, NB, words, tables=t)
    assert len({tuple(r) for r in ids.tolist()}) == NB and gum[0] == 0.0 and (np.diff(gum) <= 0).all() and np.isfinite(scores).all()
    for r in ids.tolist():
        assert [r[l * SENT + 1] for l in range(6)] == [s[0] for s in acro] and template_violations(r, t, 0) == []
        assert L.line_lengths_of(r) == [7] * 6
    for r in range(NB):
        assert abs(teacher_forced_score(w, sh, table, start_row(batch, 0), ids[r], tables=t) - float(scores[r])) < 1e-3 + 2e-5 * abs(float(scores[r]))


def test_one_row_is_ancestral_sampling_by_the_gumbel_max_trick():
    """nb = 1: every free column holds argmax_v (log p_v + n_v), the row's gum stays 0 and its score is the log-probability of what
    it drew."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    words = stochastic_row_seeds(3, 0, 1, 1)
    ids, scores, gum, gaps = cpu_stochastic_beam_search(w, sh, table, start_row(batch, 0), 44, 1, words)
    assert gum[0] == 0.0 and np.isfinite(scores[0]) and all(g > 0 for _, g in gaps)
    base, cf = _base(start_row(batch, 0)), O.CachedForward(w, sh, table)
    for c in range(1, 45):
        if c % SENT in (0, SENT - 1):
            continue
        x, only = _column(cf, base, ids[0, :c].tolist(), c, 160, None, 0, 0)
        if x is None:
            continue
        lp = x - (np.log(np.exp(x[np.isfinite(x)] - x[np.isfinite(x)].max()).sum()) + x[np.isfinite(x)].max())
        t = np.where(np.isfinite(x), lp + gumbel_noise(words, sh.P + c - 1, 160)[0], -np.inf)
        assert ids[0, c] == int(np.argmax(t))
    ids2 = cpu_stochastic_beam_search(w, sh, table, start_row(batch, 0), 44, 1, stochastic_row_seeds(4, 0, 1, 1))[0]
    assert not np.array_equal(ids, ids2)


# ------------------------------------------------------------------ the inputs of the kernel test, and their float64 answers
# 10 x the worst fp32 errors tools/stochastic_fp32_bands.py reports (t 5.4e-6, lp 3.8e-6, cand_g 4.1e-5), rounded up to one digit
T_BAND, LP_BAND, G_BAND = 6e-5, 4e-5, 5e-4
KERNEL_V, KERNEL_NB, KERNEL_ROWS = (103, 104, 1000, 13317), (1, 4, 16), 64
KP, KPOS, KNGRAM = 5, 5 + 29, 2            # the step appends lyric column j = 30: line 1, content column 7
# rows with a rule of their own (every other row: the n-gram ban and the penalty alone)
ROW_PAD_BANNED, ROW_FULL_LINE, ROW_BIGRAM, ROW_GIVEN, ROW_STICKY, ROW_DEAD_GUM, ROW_DEAD_SCORE, ROW_ALL_BANNED, ROW_COPY, ROW_HELD, ROW_CLASS = range(3, 14)


def processed_row(logits32, gen, V, ngram, pad_banned, cls, temperature=T, rep=REP):
    """The processed logits of the candidates kernels for one row, fp32 arithmetic in their order (one division per occurrence, then
    the temperature), as float64: gen the row's lyric columns so far, cls a bool [V] class mask or None."""
    f = np.float32
    x = logits32[:V].astype(f).copy()
    cnt = np.bincount([v for v in gen if 0 <= v < V], minlength=V)
    cnt[0] = 0                                                      # PAD is never penalised
    for i in range(int(cnt.max())):
        x = np.where(cnt > i, (x / f(rep)).astype(f), x)
    x = (x / f(temperature)).astype(f).astype(np.float64)
    x[[v for v in (1, 2, 100, 102) if v < V]] = -np.inf
    x[sorted(v for v in banned_ids(gen, ngram) if v < V)] = -np.inf
    if cls is not None:
        x[1:][~cls[1:]] = -np.inf
    if pad_banned:
        x[0] = -np.inf
    return x


@functools.lru_cache(maxsize=None)
def kernel_case(V):
    """64 rows at one step for vocabulary cut V (host arrays): logits, histories, the refrain form's tables, the rows' state -- and what
    float64 says of them: x [64, V] processed logits, only [64] (the id of a single-choice row, else -1), held (rows that write
    nothing)."""
    rng = np.random.default_rng(V)
    B, P, pos, n_lines = KERNEL_ROWS, KP, KPOS, 4
    j = pos + 1 - P
    ldl, ldseq = V + 5, P + 3 * SENT
    content = np.array([v for v in range(3, V) if v not in (100, 102)])
    logits = (rng.normal(0.0, 2.0, (B, ldl))).astype(np.float32)
    seq = np.zeros((B, ldseq), np.int64)
    seq[:, :P] = rng.integers(3, 99, (B, P))
    gen = rng.choice(content[:40], (B, j))                          # few ids: the penalty counts several occurrences
    gen[:, 0], gen[:, SENT - 1], gen[:, SENT] = 1, 2, 1
    gen[ROW_STICKY, j - 1] = 0
    gen[ROW_BIGRAM, j - 1], gen[ROW_BIGRAM, 3:5] = content[7], content[[7, 9]]        # (7, 9) is held: 9 is banned after 7
    seq[:, P:P + j] = gen
    lo, hi = np.zeros((B, n_lines), np.uint8), np.full((B, n_lines), SENT - 2, np.uint8)
    lo[ROW_PAD_BANNED, 1] = lo[ROW_ALL_BANNED, 1] = 10
    hi[ROW_FULL_LINE, 1] = 7
    words32 = (V + 31) // 32
    cls = np.zeros((2, V), bool)                                    # class 0: no id at all; class 1: every third content id
    cls[1, content[::3]] = True
    sets = np.zeros((2, words32), np.uint32)
    for v in np.flatnonzero(cls[1]):
        sets[1, v >> 5] |= np.uint32(1 << (v & 31))
    set_of = np.full((B, n_lines), -1, np.int16)
    tmpl = np.full((B, n_lines, SENT - 2), -1, np.int32)
    tmpl[ROW_GIVEN, 1, 7], tmpl[ROW_ALL_BANNED, 1, 7], tmpl[ROW_CLASS, 1, 7] = content[11], -2, -3
    src = np.full((B, n_lines), -1, np.int8)
    src[ROW_COPY, 1] = 0
    fixed_end = np.zeros(B, np.int32)
    fixed_end[ROW_HELD] = pos + 2
    scores, gum = (-rng.random(B) * 40.0).astype(np.float32), (-rng.random(B) * 5.0).astype(np.float32)
    gum[::8] = 0.0
    gum[ROW_DEAD_GUM], scores[ROW_DEAD_SCORE] = -np.inf, -np.inf
    words = stochastic_row_seeds(V, 0, B, 1)
    x, only = np.full((B, V), -np.inf), np.full(B, -1)
    only[[ROW_FULL_LINE, ROW_GIVEN, ROW_STICKY, ROW_COPY]] = [0, content[11], 0, gen[ROW_COPY, j - SENT]]
    for b in range(B):
        if only[b] < 0:
            x[b] = processed_row(logits[b], gen[b].tolist(), V, KNGRAM, b in (ROW_PAD_BANNED, ROW_ALL_BANNED),
                                 cls[0] if b == ROW_ALL_BANNED else cls[1] if b == ROW_CLASS else None)
    assert not np.isfinite(x[ROW_ALL_BANNED]).any() and np.isneginf(x[ROW_BIGRAM, content[9]]) and np.isneginf(x[ROW_PAD_BANNED, 0])
    return dict(V=V, B=B, P=P, pos=pos, ldl=ldl, logits=logits, seq=seq, lo=lo, hi=hi, sets=sets.view(np.int32), set_of=set_of, tmpl=tmpl,
                src=src, fixed_end=fixed_end, scores=scores, gum=gum, words=words, x=x, only=only, held=[ROW_HELD],
                nothing=[ROW_DEAD_GUM, ROW_DEAD_SCORE, ROW_ALL_BANNED])


@functools.lru_cache(maxsize=None)
def kernel_answers(V, nb):
    """constraints.gumbel_candidates on kernel_case(V): (cand_id, cand_val, cand_g, the deciding gap per row)."""
    c = kernel_case(V)
    gaps = []
    ids, val, g = gumbel_candidates(c["x"], c["scores"], c["gum"], c["words"], c["pos"], nb, only=c["only"], gaps=gaps)
    return ids, val, g, np.array(gaps)


def test_the_kernel_test_inputs_leave_at_most_a_tenth_of_the_rows_inside_the_band():
    """With the restatement alone: per case of tests/test_stochastic_gpu.py's kernel test, the rows whose nb-th / (nb + 1)-th t lie
    within T_BAND of each other (there fp32 may offer another id) are at most 10 % of the 64."""
    for V in KERNEL_V:
        for nb in KERNEL_NB:
            gaps = kernel_answers(V, nb)[3]
            assert (gaps <= T_BAND).sum() <= KERNEL_ROWS // 10, (V, nb, int((gaps <= T_BAND).sum()))
