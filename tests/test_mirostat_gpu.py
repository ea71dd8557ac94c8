"""Mirostat v2 on the MI355X: mmtg_logits_process_sample_mirostat against the float64 restatement (constraints.mirostat_filter /
mirostat_update, which tests/test_mirostat_cpu.py holds to a transcription of llama.cpp's rule) on rows chosen to clear the fp32
bands, one step and over forty; the control on the device; sampled generations of the tiny model against a host loop on the tapped
logits with the decoder's own uniforms and the device's own mu; graph replay against eager execution; the eta = 0 and tau = 32 limits;
off-means-off; the text surface.

The bands.  The device works in fp32.  tools/mirostat_fp32_bands.py evaluates the stage's arithmetic in float32 numpy in the kernel's
order of operations (the mass m from 256 strided partial sums, the butterfly and the four waves; the cut exp2(-mu) * m; the kept mass Z
from the CDF pass's chunk sums and scan; s = (log Z - (x - max)) / ln 2; the stored mu') against float64, on 30 seeds x 3 scales x 9
values of mu at V = 257 and 500 and 3 x 3 x 3 at V = 13317.  Largest errors seen: the cut 1.94e-6 bits (how far the comparison
e >= exp2(-mu) m sits from -log2 p <= mu), s 2.07e-6 bits, one update of mu divided by eta 9.70e-6 bits at eta = 0.1 (the rounding of
the stored mu, half an ulp of a number below 32, is most of it).  With the issue's margin of 10, rounded up to one digit:
    S_BAND   = 1e-4 bits  (s, and one mu update divided by eta)
    CUT_BAND = 2e-5 bits  (the distance between -log2 p and mu inside which fp32 and float64 may disagree)
The earlier stages keep the bands of tests/test_warp_gpu.py.  The kernel tests assert that their float64 rows have no id inside a band
(the seeds were searched for that on the host) and then compare kept sets for equality; an id that holds the survivors' maximum is
kept whatever its surprise and is not held against the cut band."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import WARP_OFF, mirostat_filter, mirostat_update, warp_filter  # noqa: E402
from mmtg_amd.decode import GreedyDecoder  # noqa: E402
from mmtg_amd.generate import top_k_top_p_filtering  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, setup_case  # noqa: E402
from test_ngram_cpu import banned_ids  # noqa: E402
from test_ngram_gpu import build  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402
from test_warp_gpu import inside_bands, kernel_rows, warp_of  # noqa: E402

DEV = "cuda"
S_BAND = 1e-4
CUT_BAND = 2e-5
TAU, ETA = 2.0, 0.1
MU_SPREAD = (1.0, 3.0, 6.0, 12.0)
CONFIGS = {"alone": (0, {}), "top_k": (30, {}), "typical_p": (0, dict(typical_p=0.8)),
           "all": (0, dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=2e-3))}


def cut_distance(survivors, mu):
    """How far, in bits, the nearest survivor that does not hold the maximum lies from the cut (mirostat_filter's margins)."""
    m = []
    mirostat_filter(survivors, mu, margins=m)
    d = np.array([x[2] for x in m])
    free = survivors[survivors > -np.inf] != survivors[survivors > -np.inf].max()
    return float(d[free].min()) if free.any() else float("inf")


def host_draw(before, warp, mu, margins=None):
    """The float64 rule on a row of processed, top-k / top-p filtered logits: (the kept row or None where an id lies inside a band,
    the distance to the cut)."""
    m = []
    survivors = warp_filter(before, *warp, margins=m)
    d = cut_distance(survivors, mu)
    if margins is not None:
        margins.extend(m)
    if inside_bands(m) or d <= CUT_BAND:
        return None, d
    return mirostat_filter(survivors, mu), d


def in_cdf_interval(kept_row, pick, u, band):
    p = np.exp(kept_row - kept_row[kept_row > -np.inf].max())
    cdf = np.cumsum(p)
    Z = float(cdf[-1])
    return float(cdf[pick] - p[pick]) - band * Z <= u * Z <= float(cdf[pick]) + band * Z


# ------------------------------------------------------------------ 5. the kernel, one step
def host_rows(seed, V, Vpad, top_k, kw, extra):
    """The rows of test_warp_gpu.kernel_rows, mu spread over MU_SPREAD, and per row what float64 expects: None for the sticky-PAD row,
    else (processed logits, kept row or None inside a band)."""
    logits, generated, lens, u = kernel_rows(seed, V, Vpad, extra)
    mu = torch.tensor([MU_SPREAD[(b if extra else b + 2) % 4] for b in range(logits.shape[0])], dtype=torch.float32)     # (two rows: 6, 12)
    want = []
    for b in range(logits.shape[0]):
        gl = generated[b, :lens[b]]
        if int(gl[-1]) == 0:
            want.append(None)
            continue
        proc = O.process_logits(logits[b, :V], gl, T, REP)
        before = O.top_k_top_p_filtering(proc.clone(), top_k, 0.0).double().numpy()
        want.append((proc, host_draw(before, warp_of(kw), float(mu[b]))[0], int(np.isfinite(before).sum())))
    return logits, generated, lens, u, mu, want


def check_kernel(seed, V, Vpad, config, extra):
    top_k, kw = CONFIGS[config]
    logits, generated, lens, u, mu, want = host_rows(seed, V, Vpad, top_k, kw, extra)
    B, G = logits.shape[0], generated.shape[1]
    nxt = torch.full((B,), -7, dtype=torch.long, device=DEV)
    filt = torch.full((B, Vpad), float("nan"), device=DEV)
    mu_d, sur = mu.clone().to(DEV), torch.full((B,), float("nan"), device=DEV)
    hip.logits_process_sample_mirostat(logits.to(DEV), Vpad, V, generated.to(DEV), G, lens.to(DEV), T, REP, top_k, 0.0, u.to(DEV), nxt, B,
                                       TAU, ETA, mu_d, sur, *warp_of(kw), filtered=filt)
    nxt, filt, mu_d, sur = nxt.cpu(), filt.cpu(), mu_d.cpu(), sur.cpu()
    sizes = []
    for b in range(B):
        if want[b] is None:                                                      # sticky PAD: no draw, no update
            assert int(nxt[b]) == 0 and float(sur[b]) == 0.0
            assert mu_d[b].view(torch.int32) == mu[b].view(torch.int32)
            continue
        proc, f, n_before = want[b]
        assert f is not None, (b, "the precondition: float64 has no id inside a band")
        kept = torch.from_numpy(f > -np.inf)
        assert torch.equal(torch.isfinite(filt[b, :V]), kept), (b, (torch.isfinite(filt[b, :V]) != kept).nonzero().flatten()[:8])
        assert torch.equal(filt[b, :V][kept], proc[kept]) and bool((filt[b, :V][~kept] == -float("inf")).all())
        t = int(nxt[b])
        assert kept[t] and t not in (1, 2, 100, 102)
        assert in_cdf_interval(f, t, float(u[b]), 1e-5), (b, t)
        s, up = mirostat_update(f, t, float(mu[b]), TAU, ETA)
        print("row %d: mu %g, %d -> %d kept, s %.6f (device off by %.2e), mu' off by %.2e"
              % (b, float(mu[b]), n_before, int(kept.sum()), s, abs(float(sur[b]) - s), abs(float(mu_d[b]) - up)))
        assert abs(float(sur[b]) - s) <= S_BAND and abs(float(mu_d[b]) - up) <= S_BAND, (b, float(sur[b]), s, float(mu_d[b]), up)
        sizes.append((n_before, int(kept.sum())))
    return sizes


# seeds for which no row has an id inside a band in float64 (searched on the host; check_kernel asserts it)
SEEDS = {"alone": 0, "top_k": 0, "typical_p": 0, "all": 0}
SEEDS_V = {(257, "alone"): 0, (257, "all"): 0, (13317, "alone"): 0, (13317, "all"): 0}


@pytest.mark.parametrize("config", list(SEEDS))
def test_the_kernel_keeps_what_the_float64_rule_keeps_draws_from_it_and_updates_mu(config):
    """mmtg_logits_process_sample_mirostat at V = 500 / ld 512 on thirteen rows with mu spread over 1, 3, 6, 12: `filtered` has the
    float64 kept set and the oracle's processed values bit for bit, the pick lies in the float64 CDF interval within 1e-5, `surprise`
    and the new mu agree with mirostat_update within the s-band, the sticky-PAD row's mu is bit-unchanged -- the stage alone, behind
    top_k = 30, behind typical_p = 0.8 and with all four earlier stages on."""
    sizes = check_kernel(SEEDS[config], 500, 512, config, extra=True)
    assert len(sizes) == 12 and sum(k < n for n, k in sizes) >= 6                # the cut drops something on most rows
    assert len({k for _, k in sizes}) >= 4                                      # and the spread of mu shows


@pytest.mark.parametrize("V,config", list(SEEDS_V))
def test_the_kernel_at_other_vocabulary_sizes(V, config):
    sizes = check_kernel(SEEDS_V[(V, config)], V, (V + 7) // 8 * 8, config, extra=False)
    assert len(sizes) == 2 and all(k < n for n, k in sizes)


# ------------------------------------------------------------------ 6. the state over steps, stand-alone
STEPS = 40


def test_forty_launches_feed_mu_back_and_follow_the_float64_trajectory():
    """13 rows, 40 launches with fresh seeded logits, the device's mu fed back.  Every step is checked on the host from the device's
    own mu read before the step (kept set, pick, s, mu'), so nothing accumulates; a row and step with an id inside a band is set aside
    (at most 1 in 20).  At the end the device's mu is held against the pure float64 trajectory that follows the device's picks: at
    most steps * eta * s-band apart, on the rows where that trajectory kept the device's sets throughout (a row that was set aside
    once, or whose two values of mu had an id between them, may have drawn from another set and is not comparable)."""
    V, Vpad, seed = 500, 512, 0
    _, generated, lens, _ = kernel_rows(seed, V, Vpad, True)
    B, G = generated.shape
    g = torch.Generator().manual_seed(100 + seed)
    logits = torch.zeros(STEPS, B, Vpad)
    logits[:, :, :V] = torch.randn(STEPS, B, V, generator=g) * 3
    us = torch.rand(STEPS, B, generator=g).clamp_(max=1.0 - 2.0 ** -24)
    mu_d = torch.full((B,), 2 * TAU, dtype=torch.float32, device=DEV)
    sur = torch.zeros(B, device=DEV)
    nxt = torch.zeros(B, dtype=torch.long, device=DEV)
    filt = torch.zeros(B, Vpad, device=DEV)
    gen_d, lens_d = generated.to(DEV), lens.to(DEV)
    traj = np.full(B, 2 * TAU)
    comparable = np.ones(B, dtype=bool)
    checked = aside = 0
    for t in range(STEPS):
        before_mu = mu_d.cpu().clone()
        hip.logits_process_sample_mirostat(logits[t].to(DEV), Vpad, V, gen_d, G, lens_d, T, REP, 0, 0.0, us[t].to(DEV), nxt, B, TAU, ETA, mu_d,
                                           sur, filtered=filt)
        after_mu, picks, ss, fl = mu_d.cpu(), nxt.cpu(), sur.cpu(), filt.cpu()
        for b in range(B):
            gl = generated[b, :lens[b]]
            if int(gl[-1]) == 0:
                assert int(picks[b]) == 0 and after_mu[b].view(torch.int32) == before_mu[b].view(torch.int32) and float(ss[b]) == 0.0
                comparable[b] = False
                continue
            before = O.process_logits(logits[t, b, :V], gl, T, REP).double().numpy()
            f, _ = host_draw(before, WARP_OFF, float(before_mu[b]))
            if f is None:
                aside += 1
                comparable[b] = False
                continue
            pick = int(picks[b])
            assert np.array_equal(np.isfinite(fl[b, :V].numpy()), f > -np.inf), (t, b)
            assert f[pick] > -np.inf and in_cdf_interval(f, pick, float(us[t, b]), 1e-5), (t, b)
            s, up = mirostat_update(f, pick, float(before_mu[b]), TAU, ETA)
            assert abs(float(ss[b]) - s) <= S_BAND and abs(float(after_mu[b]) - up) <= S_BAND, (t, b, float(ss[b]), s)
            checked += 1
            if comparable[b]:
                ft = mirostat_filter(before, traj[b])
                if np.array_equal(ft > -np.inf, f > -np.inf):
                    traj[b] = mirostat_update(ft, pick, traj[b], TAU, ETA)[1]
                else:
                    comparable[b] = False
    final = mu_d.cpu().double().numpy()
    bound = STEPS * ETA * S_BAND
    diff = np.abs(final - traj)[comparable]
    print("checked %d, set aside %d; %d comparable rows, mu in [%.3f, %.3f], device against the float64 trajectory: at most %.3e (bound %.1e)"
          % (checked, aside, int(comparable.sum()), final.min(), final.max(), diff.max(), bound))
    assert checked > 400 and 20 * aside <= checked
    assert comparable.sum() >= 8 and diff.max() <= bound


# ------------------------------------------------------------------ 7. the control on the device
def test_the_device_holds_the_mean_surprise_at_tau():
    """tests/test_mirostat_cpu.py's simulation on the device: V = 500, fresh rows normal * 2 per launch, 64 rows, 200 launches at
    tau = 2, eta = 0.1; every row's mean surprise over launches 100 and later lies within 0.15 bits of tau."""
    V, Vpad, B, N = 500, 512, 64, 200
    rng = np.random.default_rng(11)
    x = np.zeros((N, B, Vpad), dtype=np.float32)
    x[:, :, :V] = rng.normal(size=(N, B, V)) * 2.0
    logits = torch.from_numpy(x).to(DEV)
    us = torch.from_numpy(rng.random(size=(N, B)).astype(np.float32)).clamp_(max=1.0 - 2.0 ** -24).to(DEV)
    generated = torch.ones(B, 1, dtype=torch.long, device=DEV)
    lens = torch.ones(B, dtype=torch.int32, device=DEV)
    mu = torch.full((B,), 2 * TAU, dtype=torch.float32, device=DEV)
    sur = torch.zeros(N, B, device=DEV)
    nxt = torch.zeros(B, dtype=torch.long, device=DEV)
    for t in range(N):
        hip.logits_process_sample_mirostat(logits[t], Vpad, V, generated, 1, lens, 1.0, 1.0, 0, 0.0, us[t], nxt, B, TAU, ETA, mu, sur[t])
    means = sur[100:].mean(0).cpu().numpy()
    print("mean surprise over launches 100.. in [%.4f, %.4f], worst distance from tau %.4f; first launches %.2f bits"
          % (means.min(), means.max(), np.abs(means - TAU).max(), float(sur[:3].mean())))
    assert np.abs(means - TAU).max() <= 0.15


# ------------------------------------------------------------------ 8. generations against a host loop
def follow_the_host_loop(dec, tb, length, kw, seed, prefix=None, n=0, tau=TAU, eta=ETA):
    """test_warp_gpu.follow_the_host_loop's scheme with the state: the tap records picks, logits, history, uniforms and a clone of
    dec.mirostat_mu after every step (before the step: the clone of the step before, 2 * tau at the start).  Every row a head step
    decided is checked from the device's mu before the step -- kept pick, the CDF interval (u Z within 1e-4 Z), and mu' within the
    s-band; a step with an id inside a band is set aside.  Every other row and step -- forced, held, PAD, a step without the head --
    has a bit-equal mu before and after.  Returns (ids, steps checked, steps set aside, unchanged rows seen)."""
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    steps = []

    def tap(j, with_head, picked, logits):
        steps.append((j, with_head, picked.cpu().tolist(), logits[:, :V].float().cpu().clone() if with_head else None,
                      dec.seq[:, P:P + j].cpu().tolist(), dec.uniforms[P + j - 1].cpu().tolist(), dec.mirostat_mu.cpu().clone()))

    args = dict(temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0, no_repeat_ngram_size=n, prefix=prefix, mirostat_tau=tau,
                mirostat_eta=eta, **kw)
    ids = dec.generate(tb, length, generator=torch.Generator(device=DEV).manual_seed(seed), tap=tap, **args).cpu()
    final = dec.mirostat_mu.cpu().clone()
    checked = aside = still = 0
    prev = torch.full((dec.B,), 2.0 * tau, dtype=torch.float32)
    warp = warp_of(kw)
    for j, with_head, picked, logits, hist, us, mu_after in steps:
        for b in range(len(picked)):
            same = bool(mu_after[b].view(torch.int32) == prev[b].view(torch.int32))
            g = hist[b]
            drew = with_head and not (prefix is not None and j < len(prefix[b])) and g[-1] != 0
            if drew:
                x = O.process_logits(logits[b], torch.tensor(g), T, REP).clone()
                for v in banned_ids(g, n):
                    x[v] = float("-inf")
                drew = bool(torch.isfinite(x).any())
            if not drew:
                assert same, (j, b, "a column the row does not draw leaves mu alone")
                still += 1
                continue
            f, _ = host_draw(top_k_top_p_filtering(x.clone(), top_k=0, top_p=0.0).double().numpy(), warp, float(prev[b]))
            if f is None:
                aside += 1
                continue
            assert f[picked[b]] > -np.inf, (j, b, picked[b])
            assert in_cdf_interval(f, picked[b], us[b], 1e-4), (j, b)
            s, up = mirostat_update(f, picked[b], float(prev[b]), tau, eta)
            assert abs(float(mu_after[b]) - up) <= S_BAND, (j, b, float(mu_after[b]), up, s)
            checked += 1
        prev = mu_after
    assert torch.equal(prev, final)
    again = dec.generate(tb, length, generator=torch.Generator(device=DEV).manual_seed(seed), **args).cpu()
    assert torch.equal(ids, again) and torch.equal(dec.mirostat_mu.cpu(), final)
    return ids, checked, aside, still


def mirostat_keys(dec):
    return [k for k in dec.graphs if any(isinstance(e, tuple) and e and e[0] == "mirostat" for e in k)]


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_a_mirostat_generation_follows_the_host_rule_from_the_device_s_own_mu(mode):
    model, tb = build("tiny_s5", mode)
    length = 3 * SENT
    dec = GreedyDecoder(model, 3, max_len=length)
    plain = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0,
                         generator=torch.Generator(device=DEV).manual_seed(21)).cpu()
    assert dec.mirostat_mu is None
    for kw in (dict(), dict(typical_p=0.9)):
        ids, checked, aside, still = follow_the_host_loop(dec, tb, length, kw, seed=21)
        print(mode, kw, "checked", checked, "set aside", aside, "rows and steps that left mu alone", still, "final mu", dec.mirostat_mu.tolist())
        assert checked > 100 and 20 * aside <= checked and still >= 12
        assert not torch.equal(ids, plain)
    keys = mirostat_keys(dec)
    assert keys and all(k[0] for k in keys) and all(("mirostat", TAU, ETA) in k for k in keys)       # head steps only


def test_a_mirostat_generation_under_a_prefix_and_an_n_gram_ban_follows_the_host_rule():
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", "f32")
    dec = GreedyDecoder(model, 3, max_len=3 * SENT)
    line = batch["targets"][0, :SENT].tolist()
    pre = [line[:5], line[:3], [1]]
    ids, checked, aside, still = follow_the_host_loop(dec, tb, 3 * SENT, {}, seed=5, prefix=pre, n=2)
    print("prefix + ngram: checked", checked, "set aside", aside, "left alone", still)
    assert checked > 100 and 20 * aside <= checked and still >= 12
    for b, p in enumerate(pre):
        assert ids[b, :len(p)].tolist() == p
    assert any("prefix" in k and "ngram" in k for k in mirostat_keys(dec))


# ------------------------------------------------------------------ 9. graph replay is eager execution
def test_graph_capture_replay_and_eager_execution_agree_on_ids_and_mu():
    """A fresh decoder captures every graph key during the run: the warm-up step outside capture must not leave its update in mu
    (_step_state rewinds it).  Then the replay from the cache, then eager launches: the same ids and the same final mu, bit for bit.
    A lanes = 2 decoder over a 4-row batch against lanes = 1 likewise."""
    model, tb = build("tiny_s5", "bf16")
    length = 3 * SENT
    kw = dict(temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0, mirostat_tau=TAU, mirostat_eta=ETA)
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)                     # noqa: E731
    eager = GreedyDecoder(model, 3, max_len=length, use_graph=False)
    want = eager.generate(tb, length, generator=gen(), **kw).cpu()
    want_mu = eager.mirostat_mu.cpu().clone()
    assert not getattr(eager, "graphs", None) and float((want_mu - 2 * TAU).abs().max()) > 0.0
    dec = GreedyDecoder(model, 3, max_len=length)
    assert dec.use_graph
    first = dec.generate(tb, length, generator=gen(), **kw).cpu()                # every key captured during this run
    first_mu = dec.mirostat_mu.cpu().clone()
    assert mirostat_keys(dec)
    assert torch.equal(first, want) and torch.equal(first_mu.view(torch.int32), want_mu.view(torch.int32)), (first_mu, want_mu)
    n_keys = len(dec.graphs)
    second = dec.generate(tb, length, generator=gen(), **kw).cpu()               # replayed from the cache
    assert len(dec.graphs) == n_keys
    assert torch.equal(second, want) and torch.equal(dec.mirostat_mu.cpu().view(torch.int32), want_mu.view(torch.int32))
    third = dec.generate(tb, length, generator=gen(), use_graph=False, **kw).cpu()
    assert torch.equal(third, want) and torch.equal(dec.mirostat_mu.cpu().view(torch.int32), want_mu.view(torch.int32))
    # lanes: the fixture's rows repeated to four
    tb4 = {k: torch.cat([v, v[:1]], 0) for k, v in tb.items()}
    one, two = GreedyDecoder(model, 4, max_len=length, lanes=1), GreedyDecoder(model, 4, max_len=length, lanes=2)
    a = one.generate(tb4, length, generator=gen(), **kw).cpu()
    b = two.generate(tb4, length, generator=gen(), **kw).cpu()
    assert torch.equal(a, b) and torch.equal(one.mirostat_mu.cpu().view(torch.int32), two.mirostat_mu.cpu().view(torch.int32))
    assert two.children[1].mirostat_mu.data_ptr() == two.mirostat_mu[2:].data_ptr()      # a lane holds a view of its rows
    assert not torch.equal(a[0], a[3])                                          # (the same prompt, its own uniforms and its own mu)
    b2 = two.generate(tb4, length, generator=gen(), **kw).cpu()
    assert torch.equal(b2, a) and torch.equal(one.mirostat_mu.cpu().view(torch.int32), two.mirostat_mu.cpu().view(torch.int32))


# ------------------------------------------------------------------ 10. limits
def tapped(dec, tb, length, seed, **kw):
    """(ids, per head step and row the processed logits) of a sampled generation."""
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    rows = []

    def tap(j, with_head, picked, logits):
        if with_head:
            lg, hist = logits[:, :V].float().cpu(), dec.seq[:, P:P + j].cpu().tolist()
            for b in range(len(hist)):
                if hist[b][-1] != 0:
                    rows.append(O.process_logits(lg[b], torch.tensor(hist[b]), T, REP).double().numpy())

    ids = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0, tap=tap,
                       generator=torch.Generator(device=DEV).manual_seed(seed), **kw).cpu()
    return ids, rows


def test_eta_zero_is_the_epsilon_stage_and_tau_32_is_plain_sampling():
    model, tb = build("tiny_s5", "f32")
    length = 3 * SENT
    dec = GreedyDecoder(model, 3, max_len=length)
    # eta = 0, tau = 3: mu stays 6, the stage is epsilon_cutoff = 2^-6.  The seed is searched from the tapped logits: no step with an id
    # inside the epsilon stage's band or the cut band
    found = None
    for seed in range(1, 13):
        want, rows = tapped(dec, tb, length, seed, epsilon_cutoff=2.0 ** -6)
        clear = True
        for x in rows:
            m = []
            warp_filter(x, epsilon_cutoff=2.0 ** -6, margins=m)
            clear &= not inside_bands(m) and cut_distance(x, 6.0) > CUT_BAND
        if clear:
            found = seed
            break
    assert found is not None, "no seed in 1 .. 12 keeps every step clear of the bands"
    assert len(rows) > 100
    got = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0, mirostat_tau=3.0, mirostat_eta=0.0,
                       generator=torch.Generator(device=DEV).manual_seed(found)).cpu()
    assert torch.equal(got, want), found
    assert bool((dec.mirostat_mu == 6.0).all())
    plain, _ = tapped(dec, tb, length, found)
    assert not torch.equal(plain, want)                                         # (the cut bites)
    # tau = 32, eta = 0: mu = 64 keeps everything a plain draw can reach
    plain, rows = tapped(dec, tb, length, 3)
    for x in rows:
        logp = (x - x.max()) - np.log(np.exp(x - x.max()).sum())
        assert (logp[x > -np.inf] / np.log(2.0)).min() > -60.0                  # the precondition: no survivor below 2^-60
    got = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0, mirostat_tau=32.0, mirostat_eta=0.0,
                       generator=torch.Generator(device=DEV).manual_seed(3)).cpu()
    assert torch.equal(got, plain) and bool((dec.mirostat_mu == 64.0).all())


# ------------------------------------------------------------------ 11. off means off
def test_mirostat_tau_zero_is_exactly_the_call_without_the_arguments(monkeypatch):
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
    off = dict(mirostat_tau=0, mirostat_eta=0.1)
    runs = []
    for kw in (dict(), off, dict(mirostat_tau=0.0, mirostat_eta=0.7)):           # (eta alone turns nothing on)
        del names[:]
        dec = GreedyDecoder(model, 3, use_graph=False)
        ids = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, **kw)
        sids = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                            generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        wids = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, typical_p=0.9,
                            generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        assert dec.mirostat_mu is None
        runs.append((list(names), ids, sids, wids))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and all(torch.equal(x, y) for x, y in zip(r[1:], runs[0][1:]))
    assert not any("mirostat" in x for x in runs[0][0])
    del names[:]
    on = GreedyDecoder(model, 3, use_graph=False).generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7,
                                                           generator=torch.Generator(device=DEV).manual_seed(5), mirostat_tau=1.0)
    assert "mmtg_decode_sample_mirostat" in names
    assert not any(x.startswith("mmtg_decode_sample") and not x.endswith("_mirostat") for x in names)
    assert not torch.equal(on, runs[0][2])
    monkeypatch.undo()
    fresh, dec = GreedyDecoder(model, 3), GreedyDecoder(model, 3)
    for kw in (dict(), dict(top_k=10, top_p=0.7)):
        a = fresh.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        b = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, generator=torch.Generator(device=DEV).manual_seed(5), **kw, **off)
        assert torch.equal(a, b)
    assert set(dec.graphs) == set(fresh.graphs) and mirostat_keys(dec) == [] and dec.mirostat_mu is None
    keys = set(dec.graphs)
    dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, mirostat_tau=2.0,
                 generator=torch.Generator(device=DEV).manual_seed(5))
    new = set(dec.graphs) - keys
    assert new and set(mirostat_keys(dec)) == new and all(k[0] for k in new)     # head steps only; the others replay the graphs they had
    assert dec.mirostat_mu is not None and dec.mirostat_mu.dtype == torch.float32 and tuple(dec.mirostat_mu.shape) == (3,)
    c = dec.generate(tb, 2 * SENT, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(c, a) and dec.rules.mirostat == (0.0, 0.1) and set(dec.graphs) == keys | new


# ------------------------------------------------------------------ 12. text surface
def test_generate_samples_takes_the_arguments_ranks_and_is_deterministic_under_a_seed():
    from mmtg_amd.generate import generate_samples
    model, tb = build("tiny_s5", "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    kw = dict(n_samples=4, length=2 * SENT, top_k=0, top_p=0.0, mirostat_tau=2.0)
    texts = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), **kw)
    assert len(texts) == 3 and all(len(t) == 4 and all(isinstance(s, str) and s for s in t) for t in texts)
    again = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), **kw)
    assert again == texts
    other = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), **dict(kw, mirostat_tau=0.0))
    assert other != texts
    ranked = generate_samples(model, rows, Tok(), generator=torch.Generator(device=DEV).manual_seed(4), rank_by="mean", **kw)
    for t, r in zip(texts, ranked):
        assert sorted(t) == sorted(s for s, _, _ in r)
        means = [lp / max(cnt, 1) for _, lp, cnt in r]
        assert means == sorted(means, reverse=True) and all(np.isfinite(m) for m in means)
    with pytest.raises(ValueError, match="mirostat_tau"):
        generate_samples(model, rows, Tok(), mirostat_tau=-1)
