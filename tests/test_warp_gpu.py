"""Min-p, locally typical, epsilon and eta sampling on the MI355X: mmtg_logits_process_sample_warp against the float64 restatement
(constraints.warp_filter, which tests/test_warp_cpu.py holds to transformers' warpers) on rows chosen to clear the fp32 bands, at three
vocabulary sizes; the draw's distribution; sampled generations of the tiny model against a host loop on the tapped logits with the
decoder's own uniforms, without constraints and through the general entry's real tables; off-means-off; the greedy limits; the text
surface.

The bands (`BANDS`).  The device works in fp32, so its kept set can differ from float64's only at an id within rounding of a cut: a
probability against min_p * pmax, epsilon_cutoff or eta (relative 1e-4), a typical key against the cut key (absolute 1e-4), the
accumulated mass against typical_p (absolute 2e-5).  tools/warp_fp32_bands.py evaluates the kernel's arithmetic in float32 numpy in
the kernel's order of operations (256 strided partial sums, the butterfly, the four radix passes with the atomics in random order)
against float64, on 30 seeds x 3 scales at V = 257 and 500 and 3 x 3 at V = 13317: the largest errors seen are 4.5e-6 on the key,
6.1e-7 on the mass, 2.3e-6 relative on a probability and 6.3e-7 relative on eta -- 22x, 33x, 43x and 150x inside the bands, so the
bands stand as the issue gives them.  The kernel tests assert that their float64 rows have no id inside a band (the seeds were
searched for that on the host) and then compare kept sets for equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import WARP_OFF, warp_filter  # noqa: E402
from mmtg_amd.decode import GreedyDecoder  # noqa: E402
from mmtg_amd.generate import top_k_top_p_filtering  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, setup_case  # noqa: E402
from test_lines_cpu import apply_rule  # noqa: E402
from test_ngram_cpu import banned_ids  # noqa: E402
from test_ngram_gpu import build  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402
from test_rhyme_cpu import LENGTH, fixture_rhymes, rhyme_ends  # noqa: E402

DEV = "cuda"
NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
BANDS = {"probability": 1e-4, "key": 1e-4, "mass": 2e-5}
RULES = {"min_p": dict(min_p=0.05), "typical_p": dict(typical_p=0.9), "epsilon_cutoff": dict(epsilon_cutoff=3e-3),
         "eta_cutoff": dict(eta_cutoff=2e-3), "all": dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=2e-3)}
# behind top_k = 30 or top_p = 0.7 the survivors are the likely ids: cuts high enough to drop some of them too
BEHIND = {"min_p": dict(min_p=0.1), "typical_p": dict(typical_p=0.8), "epsilon_cutoff": dict(epsilon_cutoff=0.03),
          "eta_cutoff": dict(eta_cutoff=0.03)}


def warp_of(kw):
    return tuple({**dict(zip(NAMES, WARP_OFF)), **kw}[k] for k in NAMES)


def inside_bands(margins):
    """The (argument, kind, distance) entries of warp_filter's margins that lie inside their band."""
    return [m for m in margins if m[2] <= BANDS[m[1]]]


# ------------------------------------------------------------------ 1. / 2. the kernel against float64
def kernel_rows(seed, V, Vpad, extra, uniform=True):
    """test_logits_process_sample's nine rows (occurrence penalties, a sticky-PAD row, a three-way tie) at V = 500, or two such rows
    at another V; with `extra` four more: a uniform row, a row with one id above p = 0.999, a row of which min-p leaves one id, and a
    row whose likely ids straddle 255 / 256 and the last chunk of the CDF pass.  uniform=False (behind top_p, whose sorted cut among
    exactly equal ids is the sort's choice in the oracle and "ties stay" in the kernel, as it always was) makes the first a flat row
    of distinct values instead."""
    gen = torch.Generator().manual_seed(seed)
    B, G = (9, 40) if extra else (2, 40)
    logits = torch.zeros(B + (4 if extra else 0), Vpad)
    logits[:B, :V] = torch.randn(B, V, generator=gen) * 3
    generated = torch.randint(3, V, (logits.shape[0], G), generator=gen)
    generated[0, :10] = 7
    lens = torch.tensor([G, G, G, 1, 17, G, 5, G, 3][:B] + [1] * (logits.shape[0] - B), dtype=torch.int32)
    u = torch.tensor([0.0, 0.5, 0.123, 0.999, 0.37, 0.61, 0.05, 0.88, 0.999999][:B] + [0.3, 0.7, 0.95, 0.42][:logits.shape[0] - B],
                     dtype=torch.float32)
    if extra:
        logits[2, 10] = logits[2, 11]                    # a tie
        logits[2, 12] = logits[2, 10]
        generated[1, -1] = 0                              # sticky PAD
        generated[B:, 0] = 1                              # ([#START#]: banned anyway, so nothing of these rows is penalised)
        logits[B, :V] = 0.5                               # uniform over the 496 ids that are not banned
        if not uniform:
            logits[B, :V] += torch.randn(V, generator=gen) * 0.3
        logits[B + 1, :V] = torch.randn(V, generator=gen)
        logits[B + 1, 77] += 20.0                         # p > 0.999
        logits[B + 2, :V] = torch.randn(V, generator=gen)
        logits[B + 2, 200] = 12.0                         # the runner-up is below min_p * pmax
        logits[B + 3, :V] = torch.randn(V, generator=gen)
        logits[B + 3, 250:262] += 7.0                     # around id 255 / 256 (the strided loops' second round)
        logits[B + 3, V - 6:V] += 7.0                     # the last chunks of the CDF pass
    return logits, generated, lens, u


def check_kernel(seed, V, Vpad, top_k, top_p, kw, extra):
    logits, generated, lens, u = kernel_rows(seed, V, Vpad, extra, uniform=top_p == 0.0)
    B, G = logits.shape[0], generated.shape[1]
    warp = warp_of(kw)
    nxt = torch.full((B,), -7, dtype=torch.long, device=DEV)
    filt = torch.full((B, Vpad), float("nan"), device=DEV)
    hip.logits_process_sample_warp(logits.to(DEV), Vpad, V, generated.to(DEV), G, lens.to(DEV), T, REP, top_k, top_p, u.to(DEV), nxt, B,
                                   *warp, filtered=filt)
    nxt, filt = nxt.cpu(), filt.cpu()
    sizes, eta_branches = [], set()
    for b in range(B):
        gl = generated[b, :lens[b]]
        if int(gl[-1]) == 0:
            assert int(nxt[b]) == 0
            continue
        proc = O.process_logits(logits[b, :V], gl, T, REP)
        before = O.top_k_top_p_filtering(proc.clone(), top_k, top_p)
        margins = []
        want = warp_filter(before.double().numpy(), *warp, margins=margins)
        assert inside_bands(margins) == [], (b, inside_bands(margins))           # the precondition: float64 has no id inside a band
        kept = torch.from_numpy(want > -np.inf)
        print("row %d: %d -> %d kept, margins %s" % (b, int(torch.isfinite(before).sum()), int(kept.sum()),
                                                     ["%s/%s %.3g" % m for m in margins]))
        # (a) the restatement's kept set, the oracle's processed values bit for bit
        assert torch.equal(torch.isfinite(filt[b, :V]), kept), (b, (torch.isfinite(filt[b, :V]) != kept).nonzero().flatten()[:8])
        assert torch.equal(filt[b, :V][kept], proc[kept]) and bool((filt[b, :V][~kept] == -float("inf")).all())
        # (b) the draw: the inverse CDF of the kept softmax in index order, held to a float64 CDF with the sample test's 1e-5 band
        p64 = torch.softmax(torch.from_numpy(want), -1)
        cdf = torch.cumsum(p64, -1)
        t = int(nxt[b])
        assert kept[t] and t not in (1, 2, 100, 102)
        lo = float(cdf[t] - p64[t])
        assert lo - 1e-5 <= float(u[b]) <= float(cdf[t]) + 1e-5, (b, t, lo, float(u[b]), float(cdf[t]))
        sizes.append((int(torch.isfinite(before).sum()), int(kept.sum())))
        if warp[3] > 0.0:
            s = warp_filter(before.double().numpy(), *warp[:3])
            p = torch.softmax(torch.from_numpy(s), -1)
            H = float(-(p[p > 0] * torch.log(p[p > 0])).sum())
            eta_branches.add(bool(np.sqrt(warp[3]) * np.exp(-H) < warp[3]))
    return sizes, eta_branches


# seeds for which no row has an id inside a band in float64 (searched on the host; check_kernel asserts it)
SEEDS = {("min_p", 0, 0.0): 0, ("typical_p", 0, 0.0): 0, ("epsilon_cutoff", 0, 0.0): 0, ("eta_cutoff", 0, 0.0): 0, ("all", 0, 0.0): 2,
         ("min_p", 30, 0.0): 0, ("typical_p", 30, 0.0): 0, ("epsilon_cutoff", 30, 0.0): 0, ("eta_cutoff", 30, 0.0): 0,
         ("min_p", 0, 0.7): 1, ("typical_p", 0, 0.7): 0, ("epsilon_cutoff", 0, 0.7): 1, ("eta_cutoff", 0, 0.7): 4}
SEEDS_V = {(257, "typical_p"): 0, (257, "all"): 0, (13317, "typical_p"): 0, (13317, "all"): 0}


@pytest.mark.parametrize("rule,top_k,top_p", list(SEEDS))
def test_the_kernel_keeps_what_the_float64_restatement_keeps_and_draws_from_it(rule, top_k, top_p):
    """mmtg_logits_process_sample_warp at V = 500 / ld 512 on thirteen rows: (a) `filtered` has the float64 restatement's kept set and
    the oracle's processed values bit for bit, (b) the drawn id lies in the float64 CDF interval of the kept softmax for its uniform,
    within 1e-5 -- each rule alone, all four together, each rule behind top_k = 30 and behind top_p = 0.7.  Exact equality under the
    asserted precondition that float64 has no id inside the bands (the module docstring gives the bands and the fp32 error observed:
    key 4.5e-6, mass 6.1e-7, probabilities 2.3e-6 relative)."""
    plain = top_k == 0 and top_p == 0.0
    sizes, eta_branches = check_kernel(SEEDS[(rule, top_k, top_p)], 500, 512, top_k, top_p, (RULES if plain else BEHIND)[rule], extra=True)
    assert len(sizes) == 12 and sum(k < n for n, k in sizes) >= 3               # the stages drop something, on several rows
    if rule in ("typical_p", "epsilon_cutoff", "eta_cutoff") and plain:
        assert sizes[8] == (496, 496)                                           # the uniform row: every key ties, everybody holds the maximum
    if rule in ("min_p", "all"):
        assert sizes[10][1] == 1                                                # min-p leaves one id
    if rule in ("eta_cutoff", "all") and plain:
        assert eta_branches == {True, False}                                    # eta took its sqrt branch (high entropy) and its flat one


@pytest.mark.parametrize("V,rule", list(SEEDS_V))
def test_the_kernel_at_other_vocabulary_sizes(V, rule):
    """The same check on two rows at V = 257 (one id past the strided loops' first round, a last CDF chunk of one id) and at the
    production cut V = 13317."""
    sizes, _ = check_kernel(SEEDS_V[(V, rule)], V, (V + 7) // 8 * 8, 0, 0.0, RULES[rule], extra=False)
    assert len(sizes) == 2 and all(k < n for n, k in sizes)


# ------------------------------------------------------------------ 3. the draw's distribution
def test_twenty_thousand_draws_under_typical_p_follow_the_kept_softmax():
    """20 000 draws of one row under typical_p = 0.5: chi-square against the kept softmax below the 0.1 % quantile for the kept count's
    degrees of freedom, and nothing outside the kept set is ever drawn."""
    from scipy.stats import chi2 as chi2_dist
    V, Vpad, N = 300, 304, 20000
    g = torch.Generator().manual_seed(3)
    row = torch.zeros(Vpad)
    row[:V] = torch.randn(V, generator=g) * 2
    logits = row.repeat(N, 1).to(DEV)
    generated = torch.full((N, 1), 1, dtype=torch.long, device=DEV)
    lens = torch.ones(N, dtype=torch.int32, device=DEV)
    u = torch.rand(N, generator=g).to(DEV)
    nxt = torch.empty(N, dtype=torch.long, device=DEV)
    hip.logits_process_sample_warp(logits, Vpad, V, generated, 1, lens, 1.0, 1.0, 0, 0.0, u, nxt, N, typical_p=0.5)
    margins = []
    want = warp_filter(O.process_logits(row[:V], torch.tensor([1]), 1.0, 1.0).double().numpy(), typical_p=0.5, margins=margins)
    assert inside_bands(margins) == []
    p = torch.softmax(torch.from_numpy(want), -1)
    counts = torch.bincount(nxt.cpu(), minlength=V).double()
    kept = p > 0
    assert 3 <= int(kept.sum()) < V - 4 and float(counts[~kept].sum()) == 0
    chi2 = float((((counts[kept] - N * p[kept]) ** 2) / (N * p[kept])).sum())
    bound = float(chi2_dist.ppf(0.999, int(kept.sum()) - 1))
    print("kept %d, chi-square %.2f, bound %.2f" % (int(kept.sum()), chi2, bound))
    assert chi2 < bound, (chi2, bound)


# ------------------------------------------------------------------ 4. / 5. sampled generations against a host loop
def follow_the_host_loop(dec, tb, length, kw, seed, rule_of=None, prefix=None, n=0, **gen_kw):
    """A sampled generation with the cuts kw, and for every step that called the head and every row the step decided: the pick lies in
    the inverse-CDF interval (ids in index order, the decoder's own uniform of that position and row) of the step's tapped logits
    processed on the host -- penalty / temperature / fixed bans (the oracle's process_logits), the n-gram bans, rule_of's line rule,
    the reference's top-k / top-p filter, then the float64 restatement of the four stages.  The interval is held to the fp32 rounding
    of the CDF as in test_lines_gpu (u Z within 1e-4 Z).  A step at which float64 has an id inside a band is set aside (the device may
    keep it or not there) and counted; the callers allow one step in twenty: with 160 ids a row has some id inside a band at about
    160 x (2 x 2e-5 of accumulated mass + 2 x 1e-4 of key at under one id per unit of key per id + 2e-4 of relative probability), 2 to
    3 % of the steps.  Returns (ids, steps checked, steps set aside)."""
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    steps = []

    def tap(j, with_head, picked, logits):
        if with_head:
            steps.append((j, picked.cpu().tolist(), logits[:, :V].float().cpu().clone(), dec.seq[:, P:P + j].cpu().tolist(),
                          dec.uniforms[P + j - 1].cpu().tolist()))

    top_k, top_p = gen_kw.pop("top_k", 0), gen_kw.pop("top_p", 0.0)
    args = dict(temperature=T, repitition_penalty=REP, top_k=top_k, top_p=top_p, no_repeat_ngram_size=n, prefix=prefix, **kw, **gen_kw)
    ids = dec.generate(tb, length, generator=torch.Generator(device=DEV).manual_seed(seed), tap=tap, **args).cpu()
    checked = aside = 0
    for j, picked, logits, hist, us in steps:
        for b in range(len(picked)):
            g = hist[b]
            if prefix is not None and j < len(prefix[b]):
                assert picked[b] == prefix[b][j]
                continue
            if g[-1] == 0:
                assert picked[b] == 0
                continue
            x = O.process_logits(logits[b], torch.tensor(g), T, REP).clone()
            for v in banned_ids(g, n):
                x[v] = float("-inf")
            if rule_of is not None:
                x = rule_of(x, g, b, j)
            if x is None or not torch.isfinite(x).any():
                assert picked[b] == 0
                continue
            f = top_k_top_p_filtering(x.clone(), top_k=top_k, top_p=top_p)
            margins = []
            w = torch.from_numpy(warp_filter(f.double().numpy(), **kw, margins=margins))
            if inside_bands(margins):
                aside += 1
                continue
            assert torch.isfinite(w[picked[b]]), (j, b, picked[b])
            p = torch.exp(w - w.max())
            cdf = torch.cumsum(p, 0)
            Z, target = float(cdf[-1]), us[b] * float(cdf[-1])
            assert float(cdf[picked[b]] - p[picked[b]]) - 1e-4 * Z <= target <= float(cdf[picked[b]]) + 1e-4 * Z, (j, b)
            checked += 1
    again = dec.generate(tb, length, generator=torch.Generator(device=DEV).manual_seed(seed), **args).cpu()
    assert torch.equal(ids, again)
    return ids, checked, aside


def warp_keys(dec):
    return [k for k in dec.graphs if any(isinstance(e, tuple) and e and e[0] == "warp" for e in k)]


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_sampling_with_each_rule_follows_the_host_restatement_with_the_same_uniforms(mode):
    model, tb = build("tiny_s5", mode)
    length = 3 * SENT
    dec = GreedyDecoder(model, 3, max_len=length)
    plain = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0,
                         generator=torch.Generator(device=DEV).manual_seed(21)).cpu()
    for rule in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"):
        ids, checked, aside = follow_the_host_loop(dec, tb, length, RULES[rule], seed=21)
        print(mode, rule, "checked", checked, "set aside", aside)
        assert checked > 100 and 20 * aside <= checked
        assert not torch.equal(ids, plain)                                       # the cut changes what the same uniforms draw
    keys = warp_keys(dec)
    assert len({e for k in keys for e in k if isinstance(e, tuple) and e[0] == "warp"}) == 4 and all(k[0] for k in keys)   # head steps only


@pytest.mark.parametrize("kw", [dict(typical_p=0.9, min_p=0.05), dict(epsilon_cutoff=3e-3, eta_cutoff=2e-3)],
                         ids=["typical+min_p", "epsilon+eta"])
def test_sampling_with_the_rules_under_constraints_follows_the_host_restatement(kw):
    """The general entry with real tables: under a prefix with no_repeat_ngram_size = 2, and under line bounds with a rhyme scheme."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", "f32")
    dec = GreedyDecoder(model, 3, max_len=LENGTH)
    line = batch["targets"][0, :SENT].tolist()
    pre = [line[:5], line[:3], [1]]
    ids, checked, aside = follow_the_host_loop(dec, tb, 3 * SENT, kw, seed=5, prefix=pre, n=2)
    print("prefix + ngram: checked", checked, "set aside", aside)
    assert checked > 80 and 20 * aside <= checked
    for b, p in enumerate(pre):
        assert ids[b, :len(p)].tolist() == p
    assert any("prefix" in k and "ngram" in k for k in warp_keys(dec))
    classes, bounds = fixture_rhymes(fx)
    from mmtg_amd.decode import check_lines
    tabs = check_lines(bounds, None, 3, LENGTH, SENT, 160, rhyme_scheme="AABB", rhyme_classes=classes, rhyme_distinct=True)
    followers = [0]

    def rule_of(x, g, b, j):
        lo, hi, e = tabs.bounds(b, j // SENT)
        r = rhyme_ends(g, tabs, b)
        if r is not None:
            e, followers[0] = r, followers[0] + 1
        return apply_rule(x, g, lo, hi, e)

    ids, checked, aside = follow_the_host_loop(dec, tb, LENGTH, kw, seed=7, rule_of=rule_of, line_lengths=bounds, rhyme_scheme="AABB",
                                               rhyme_classes=classes, rhyme_distinct=True)
    print("lines + rhyme: checked", checked, "set aside", aside, "followers", followers[0])
    assert checked > 50 and 20 * aside <= checked and followers[0] > 10
    assert any("rhyme" in k and "distinct" in k for k in warp_keys(dec))


# ------------------------------------------------------------------ 6. off means off
def test_the_four_defaults_are_exactly_the_call_without_the_arguments(monkeypatch):
    model, tb = build("tiny_s5", "bf16")
    names = []
    real = hip.lib()

    class Lib:
        def __getattr__(self, name):
            f = getattr(real, name)
            if name.startswith("mmtg_decode_select") or name.startswith("mmtg_decode_sample"):
                def entry(*a):
                    names.append(name)
                    return f(*a)
                return entry
            return f
    rec = Lib()
    monkeypatch.setattr(hip, "lib", lambda: rec)
    off = dict(min_p=0, typical_p=1, epsilon_cutoff=0, eta_cutoff=0)
    runs = []
    for kw in (dict(), off):
        del names[:]
        dec = GreedyDecoder(model, 3, use_graph=False)
        ids = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, **kw)
        sids = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                            generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        runs.append((list(names), ids, sids))
    assert runs[0][0] == runs[1][0] and not any("warp" in x for x in runs[0][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    del names[:]
    on = GreedyDecoder(model, 3, use_graph=False).generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                                                           generator=torch.Generator(device=DEV).manual_seed(5), typical_p=0.5)
    assert "mmtg_decode_sample_warp" in names and not any(x.startswith("mmtg_decode_sample") and not x.endswith("_warp") for x in names)
    assert not torch.equal(on, runs[0][2])
    monkeypatch.undo()
    fresh, dec = GreedyDecoder(model, 3), GreedyDecoder(model, 3)
    for kw in (dict(), dict(top_k=10, top_p=0.7)):
        a = fresh.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        b = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, generator=torch.Generator(device=DEV).manual_seed(5), **kw, **off)
        assert torch.equal(a, b)
    assert set(dec.graphs) == set(fresh.graphs) and warp_keys(dec) == []
    keys = set(dec.graphs)
    dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, min_p=0.05,
                 generator=torch.Generator(device=DEV).manual_seed(5))
    new = set(dec.graphs) - keys
    assert new and set(warp_keys(dec)) == new and all(k[0] for k in new)         # head steps only; the others replay the graphs they had
    c = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(c, a) and dec.rules.warp == WARP_OFF


# ------------------------------------------------------------------ 7. the greedy limits
SHARP = 0.02
MIN_LIMIT_STEPS = 20


def test_typical_p_at_1e_6_and_min_p_at_1_are_the_greedy_decoder_whatever_the_uniforms():
    """typical_p = 1e-6 keeps one id, the one whose surprise is nearest the entropy.  That is the most probable id where the model is
    confident (p_max near 1: H near 0, every other id's surprise far above it) and not in general: on the tiny model at temperature
    1.1 the float64 rule -- transformers' TypicalLogitsWarper's -- keeps another id than the arg-max at every one of the 161 steps
    that call the head, and at temperature 0.1 at about half of them.  So the limit is taken at temperature 0.02, step by step:
    the sampled generation is teacher-forced onto the greedy decoder's ids (the hook of tests/test_decode_gpu.py), so every step sees
    the greedy history, and wherever the float64 restatement on the step's tapped logits keeps the arg-max alone the step's own pick
    is the greedy decoder's id, for two sets of uniforms; everywhere else the pick is the one id the restatement keeps.  A step with
    an id inside a band is set aside.  min_p = 1 keeps the ids that hold the maximum at any temperature: the greedy decoder's output
    throughout, at temperature 1.1, behind any top_k / top_p."""
    model, tb = build("tiny_s5", "f32")
    length = 3 * SENT
    dec = GreedyDecoder(model, 3, max_len=length)
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    greedy = dec.generate(tb, length, temperature=SHARP, repitition_penalty=REP).cpu()
    for seed in (1, 2):
        steps = []

        def tap(j, with_head, picked, logits):
            if with_head:
                steps.append((j, picked.cpu().tolist(), logits[:, :V].float().cpu().clone(), dec.seq[:, P:P + j].cpu().tolist()))

        dec.generate(tb, length, temperature=SHARP, repitition_penalty=REP, top_k=0, top_p=0.0, typical_p=1e-6, teacher=greedy, tap=tap,
                     generator=torch.Generator(device=DEV).manual_seed(seed))
        limit = other = aside = 0
        for j, picked, logits, hist in steps:
            for b in range(3):
                assert hist[b] == greedy[b, :j].tolist()
                if hist[b][-1] == 0:
                    assert picked[b] == 0
                    continue
                x = O.process_logits(logits[b], torch.tensor(hist[b]), SHARP, REP).double().numpy()
                margins = []
                kept = np.flatnonzero(warp_filter(x, typical_p=1e-6, margins=margins) > -np.inf).tolist()
                if inside_bands(margins):
                    aside += 1
                    continue
                assert kept == [picked[b]], (seed, j, b, kept, picked[b])
                if kept == [int(np.argmax(x))]:
                    assert picked[b] == int(greedy[b, j])
                    limit += 1
                else:
                    other += 1
        print("seed %d: the arg-max alone at %d steps (the greedy id each time), another single id at %d, set aside %d"
              % (seed, limit, other, aside))
        assert limit >= MIN_LIMIT_STEPS and 20 * aside <= limit + other
    want = dec.generate(tb, length, temperature=T, repitition_penalty=REP).cpu()
    for seed in (1, 2):
        for kw in (dict(top_k=0, top_p=0.0), dict(top_k=1, top_p=0.0), dict(top_k=10, top_p=0.7)):
            ids = dec.generate(tb, length, temperature=T, repitition_penalty=REP, min_p=1.0,
                               generator=torch.Generator(device=DEV).manual_seed(seed), **kw).cpu()
            assert torch.equal(ids, want), (seed, kw)


# ------------------------------------------------------------------ 8. text surface
def test_generate_samples_takes_the_arguments_ranks_and_is_deterministic_under_a_seed():
    from mmtg_amd.generate import generate_samples
    model, tb = build("tiny_s5", "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    kw = dict(n_samples=4, length=2 * SENT, top_k=0, top_p=0.0, typical_p=0.9, min_p=0.05)
    texts = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), **kw)
    assert len(texts) == 3 and all(len(t) == 4 and all(isinstance(s, str) and s for s in t) for t in texts)
    again = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), **kw)
    assert again == texts
    other = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), **dict(kw, typical_p=1.0, min_p=0.0))
    assert other != texts
    ranked = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), rank_by="mean", **kw)
    for t, r in zip(texts, ranked):
        assert sorted(t) == sorted(s for s, _, _ in r)
        means = [lp / max(cnt, 1) for _, lp, cnt in r]
        assert means == sorted(means, reverse=True) and all(np.isfinite(m) for m in means)
    with pytest.raises(ValueError, match="typical_p"):
        generate_samples(model, rows, Tok(), typical_p=0.0)
