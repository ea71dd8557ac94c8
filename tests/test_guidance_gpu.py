"""Classifier-free guidance on the MI355X: mmtg_decode_guidance against the float64 restatement (constraints.guidance_scores, which
tests/test_guidance_cpu.py holds to transformers) under the band stated there, on both load paths; mmtg_decode_mirror; guided
generations of the tiny model against a host loop on the tapped logits, greedy and sampled with the decoder's own uniforms; the
structure of a guided generation (the halves on one text, capture against eager, graph keys, permutation); the text surface.

The band: |device - float64| <= K_BAND * 2^-24 * (1 + 2 s) * M per pair (tests/test_guidance_cpu.py gives M, the transcription's
worst error and why K_BAND is 3)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import guidance_scores  # noqa: E402
from mmtg_amd.decode import GreedyDecoder, GuidedDecoder  # noqa: E402
from mmtg_amd.generate import without_experience  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, setup_case, start_row  # noqa: E402
from test_guidance_cpu import K_BAND, SCALES, bands, pairs_for  # noqa: E402
from test_guidance_cpu import zeroed as zeroed_row  # noqa: E402
from test_ngram_gpu import build  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402

DEV = "cuda"
ATOL = 1e-4     # tests/test_logprob_gpu.py's
NINF = float("-inf")
_MODELS = {}


def tiny(mode):
    if mode not in _MODELS:
        _MODELS[mode] = build("tiny_s5", mode)
    return _MODELS[mode]


def rolled(tb):
    return {k: torch.roll(v, 1, 0) for k, v in tb.items()}


def zeroed(tb):
    return {k: v.to(DEV) for k, v in without_experience({k: v.cpu().numpy() for k, v in tb.items()}).items()}


# ------------------------------------------------------------------ 1. the kernel against float64
def kernel_rows(V, N, seed=0):
    """N pairs of float32 rows of V ids, cycling through pairs_for's kinds (random rows at three scales, -inf holes in c only, in u
    only and in both, a one-hot and a uniform row); with N >= 3 the last pair has no distribution at all."""
    kinds = pairs_for(seed, V)
    c = np.stack([kinds[b % len(kinds)][0] for b in range(N)]).astype(np.float32)
    u = np.stack([kinds[b % len(kinds)][1] for b in range(N)]).astype(np.float32)
    if N > len(kinds):                  # (a second round of the kinds: other values)
        more = pairs_for(seed + 1, V)
        for b in range(len(kinds), N):
            c[b], u[b] = more[b % len(more)][0], more[b % len(more)][1]
    if N >= 3:
        c[N - 1] = NINF
    return c, u


WORST = {"k": 0.0}


@pytest.mark.parametrize("V", [257, 500, 13317])
@pytest.mark.parametrize("N", [1, 3, 64])
@pytest.mark.parametrize("padded", [False, True], ids=["ldl=V", "ldl=Vpad"])
def test_the_kernel_against_float64_under_the_band(V, N, padded):
    """ldl = V is odd at 257 and 13317 (rows past the first start off a 16-byte boundary: the one-logit path) and even at 500; the
    padded width is a multiple of 8 (the float4 path).  Input columns >= V hold NaN, `out` is wider than V with a sentinel in its
    padding and guard rows round it; c == u is bit-equal across the scales and a second launch repeats the first bit for bit."""
    ldl = (V + 7) // 8 * 8 if padded else V
    ldo = ldl + 8
    c, u = kernel_rows(V, N)
    cp, up = np.full((N, ldl), np.nan, np.float32), np.full((N, ldl), np.nan, np.float32)
    cp[:, :V], up[:, :V] = c, u
    dc, du = torch.from_numpy(cp).to(DEV), torch.from_numpy(up).to(DEV)
    worst = 0.0
    same = []
    for s in SCALES:
        buf = torch.full((N + 2, ldo), -77.0, device=DEV)
        out = buf[1:N + 1]
        hip.decode_guidance(dc, du, ldl, V, s, out, N)
        got = buf.cpu().numpy()
        assert (got[0] == -77.0).all() and (got[N + 1] == -77.0).all() and (got[1:N + 1, V:] == -77.0).all()
        again = torch.full((N + 2, ldo), -77.0, device=DEV)
        hip.decode_guidance(dc, du, ldl, V, s, again[1:N + 1], N)
        assert torch.equal(again, buf)
        g = got[1:N + 1, :V].astype(np.float64)
        want = guidance_scores(c, u, s)
        fin = np.isfinite(want)
        assert not np.isnan(g).any() and np.array_equal(np.isfinite(g), fin) and bool(np.isneginf(g[~fin]).all())
        for b in range(N):
            if fin[b].any():
                unit = bands.band_unit(c[b], u[b], s)
                worst = max(worst, float(np.abs(g[b][fin[b]] - want[b][fin[b]]).max() / unit))
        eq = torch.full((N, ldo), -77.0, device=DEV)
        hip.decode_guidance(dc, dc.clone(), ldl, V, s, eq, N)
        same.append(eq.cpu())
    WORST["k"] = max(WORST["k"], worst)
    print("V %d N %d ldl %d: worst error %.3f band units (K_BAND %d); worst so far %.3f" % (V, N, ldl, worst, K_BAND, WORST["k"]))
    assert worst <= K_BAND
    assert all(torch.equal(same[0], x) for x in same[1:])
    lsm = torch.log_softmax(torch.from_numpy(c.astype(np.float64)), -1).numpy()
    fin = np.isfinite(c)
    if fin.any():
        assert np.abs(same[0].numpy()[:, :V].astype(np.float64)[fin] - lsm[fin]).max() <= K_BAND * 2.0 ** -24 * 2 * (np.abs(c[fin]).max() + np.abs(lsm[fin]).max())


# ------------------------------------------------------------------ 2. the mirror
@pytest.mark.parametrize("N", [1, 5])
def test_the_mirror_writes_one_column_of_the_second_half_and_nothing_else(N):
    ld = 37
    g = torch.Generator().manual_seed(N)
    for col in (1, ld - 1, ld):
        seq = torch.randint(0, 1000, (2 * N + 1, ld), generator=g)
        dev = seq.to(DEV)
        pos = torch.tensor([col - 1], dtype=torch.int32, device=DEV)
        hip.decode_mirror(dev, pos, N)
        want = seq.clone()
        if col < ld:
            want[N:2 * N, col] = seq[:N, col]
        assert torch.equal(dev.cpu(), want) and int(pos.item()) == col - 1


# ------------------------------------------------------------------ 3. generation follows a host loop on the tapped logits
def follow_the_host_loop(dec, tb, neg, length, s, sampled, seed=3, **gen_kw):
    """A guided generation, and for every step that called the head and every prompt: guidance_scores (float64) of the two tapped
    halves goes into the oracle's process_logits and gives the pick -- greedy: the arg-max, set aside when the float64 top-2 margin is
    under 1e-3; sampled (top_k = 0, top_p = 0: every id that is not banned): the inverse-CDF interval of the decoder's own uniform, 1e-4 Z slack, as
    test_warp_gpu.follow_the_host_loop.  Returns (ids, checked, aside)."""
    P, V, n = dec.eng.sh.P, min(dec.eng.sh.V, 13317), dec.n_prompts
    steps = []

    def tap(j, with_head, picked, logits):
        if with_head:
            steps.append((j, picked.cpu().tolist(), logits[:, :V].float().cpu().numpy().copy(), dec.seq[:, P:P + j].cpu().tolist(),
                          dec.uniforms[P + j - 1].cpu().tolist() if sampled else None))

    kw = dict(temperature=T, repitition_penalty=REP, **(dict(top_k=0, top_p=0.0) if sampled else {}), **gen_kw)
    gen = lambda: torch.Generator(device=DEV).manual_seed(seed)
    ids = dec.generate(tb, neg, length, s, generator=gen(), tap=tap, **kw).cpu()
    checked = aside = 0
    for j, picked, logits, hist, us in steps:
        assert logits.shape[0] == 2 * n and picked[:n] == picked[n:] and hist[:n] == hist[n:]
        for b in range(n):
            if hist[b][-1] == 0:
                assert picked[b] == 0
                continue
            g = torch.from_numpy(guidance_scores(logits[b], logits[n + b], s))
            x = O.process_logits(g, torch.tensor(hist[b]), T, REP)
            if not sampled:
                top = torch.sort(x, descending=True, stable=True)
                if float(top.values[0] - top.values[1]) < 1e-3:
                    aside += 1
                    continue
                assert picked[b] == int(top.indices[0]), (j, b)
            else:
                p = torch.exp(x - x.max())
                cdf = torch.cumsum(p, 0)
                Z, target, t = float(cdf[-1]), us[b] * float(cdf[-1]), picked[b]
                assert torch.isfinite(x[t]) and float(cdf[t] - p[t]) - 1e-4 * Z <= target <= float(cdf[t]) + 1e-4 * Z, (j, b, t)
            checked += 1
    again = dec.generate(tb, neg, length, s, generator=gen(), **kw).cpu()
    assert torch.equal(ids, again)
    return ids, checked, aside


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("negative", ["rolled", "zeroed"])
def test_generation_follows_the_host_loop_on_the_tapped_logits(mode, negative):
    model, tb = tiny(mode)
    neg = rolled(tb) if negative == "rolled" else zeroed(tb)
    length = 3 * SENT
    dec = GuidedDecoder(model, 3, max_len=length)
    plain = GreedyDecoder(model, 3, max_len=length)
    unguided = plain.generate(tb, length, temperature=T, repitition_penalty=REP).cpu()
    unguided_s = plain.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0,
                                generator=torch.Generator(device=DEV).manual_seed(3)).cpu()
    for s in (3.0, 7.5):
        ids, checked, aside = follow_the_host_loop(dec, tb, neg, length, s, sampled=False)
        print(mode, negative, s, "greedy: checked", checked, "set aside", aside)
        assert checked > 100 and 20 * aside <= checked + aside
        assert ids.shape == (3, 1 + length) and not torch.equal(ids, unguided)
        sids, checked, aside = follow_the_host_loop(dec, tb, neg, length, s, sampled=True)
        print(mode, negative, s, "sampled: checked", checked, "set aside", aside)
        assert checked > 100 and 20 * aside <= checked + aside
        assert not torch.equal(sids, unguided_s)


# ------------------------------------------------------------------ 4. against the oracle end to end
@pytest.mark.parametrize("negative", ["rolled", "zeroed"])
def test_the_guided_step_against_the_oracle_teacher_forced_on_the_devices_history(negative):
    """f32, tiny_s5, s = 3: at every step that called the head the oracle -- two CachedForwards per prompt, one on the prompt's row and
    one on its negative's, both fed the device's own lyric history -- gives both logits rows.  The device's tapped rows lie within 1e-3
    of them (the mode's gate), and the device's pick is the arg-max of the oracle's processed guided scores wherever their float64
    top-2 margin exceeds 2 (1 + 2 s) (REP / T) x the step's observed logit difference: a difference d in a raw logit moves a guided
    score by at most (1 + 2 s) d twice over (the row and its log-sum-exp), and the penalty and the temperature scale it by at most
    REP / T.  Steps below that are set aside; the cap is one in twenty.  This holds the 2 N-row step to a model of its own: the
    concatenated batch, the negatives' conditioning rows and the mirror that feeds the next step's keys."""
    s, n, length = 3.0, 3, 3 * SENT
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = tiny("f32")
    neg = rolled(tb) if negative == "rolled" else zeroed(tb)
    dec = GuidedDecoder(model, n, max_len=length)
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    steps = []

    def tap(j, with_head, picked, logits):
        if with_head:
            steps.append((j, picked.cpu().tolist(), logits[:, :V].double().cpu().numpy().copy(), dec.seq[:n, P:P + j].cpu().tolist()))

    ids = dec.generate(tb, neg, length, s, temperature=T, repitition_penalty=REP, tap=tap).cpu()

    def base(row):
        b = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in row.items()}
        b["topic_ids"] = b["topic_ids"].long()
        return b
    rows = [start_row(batch, b) for b in range(n)]
    negs = [rows[(b - 1) % n] for b in range(n)] if negative == "rolled" else [zeroed_row(r) for r in rows]
    sides = [((O.CachedForward(w, sh, table), base(rows[b])), (O.CachedForward(w, sh, table), base(negs[b]))) for b in range(n)]
    checked = aside = 0
    worst = 0.0
    for j, picked, logits, hist in steps:
        for b in range(n):
            assert hist[b] == ids[b, :j].tolist()
            t = torch.tensor([hist[b]], dtype=torch.long)
            c, u = (cf(dict(inp, targets=t))[0, -1, :V].double().numpy() for cf, inp in sides[b])
            d = max(float(np.abs(logits[b] - c).max()), float(np.abs(logits[n + b] - u).max()))
            worst = max(worst, d)
            assert d <= 1e-3, (j, b, d)
            if hist[b][-1] == 0:
                assert picked[b] == 0
                continue
            x = O.process_logits(torch.from_numpy(guidance_scores(c, u, s)), torch.tensor(hist[b]), T, REP)
            top = torch.sort(x, descending=True, stable=True)
            if float(top.values[0] - top.values[1]) <= 2 * (1 + 2 * s) * (REP / T) * d:
                aside += 1
                continue
            assert picked[b] == int(top.indices[0]), (j, b, d)
            checked += 1
    print("oracle end to end,", negative, "negative: checked", checked, "set aside", aside, "worst logit difference %.3g" % worst)
    assert checked > 100 and 20 * aside <= checked + aside


# ------------------------------------------------------------------ 5. structure
def test_the_halves_stay_on_one_text_under_every_rule_and_capture_is_eager():
    model, tb = tiny("f32")
    length = 4 * SENT
    P = model.engine().sh.P
    line = [1, 7, 9, 11, 13]
    rules = [dict(), dict(prefix=[line, line[:3], [1]]), dict(templates=[(7, Ellipsis), (9, Ellipsis)]),
             dict(refrain_scheme="AB.A", no_repeat_ngram_size=3), dict(top_k=10, top_p=0.7, min_p=0.05)]
    dec = GuidedDecoder(model, 3, max_len=length)
    for kw in rules:
        gen = lambda: torch.Generator(device=DEV).manual_seed(11)
        ids = dec.generate(tb, rolled(tb), length, 3.0, temperature=T, repitition_penalty=REP, generator=gen(), **kw)
        cols = slice(P, P + 1 + length)
        assert torch.equal(dec.seq[:3, cols], dec.seq[3:, cols]) and torch.equal(dec.keep[:3, cols], dec.keep[3:, cols])
        assert torch.equal(ids, dec.seq[:3, cols])
        if "prefix" in kw:
            for b, p in enumerate(kw["prefix"]):
                assert ids[b, :len(p)].tolist() == p
        eager = dec.generate(tb, rolled(tb), length, 3.0, temperature=T, repitition_penalty=REP, generator=gen(), use_graph=False, **kw)
        assert torch.equal(ids, eager), kw


def test_graph_keys_the_identical_negative_and_a_permutation_of_the_prompts():
    model, tb = tiny("f32")
    length = 2 * SENT
    dec = GuidedDecoder(model, 3, max_len=length)
    kw = dict(temperature=T, repitition_penalty=REP)
    a3 = dec.generate(tb, zeroed(tb), length, 3.0, **kw)
    keys3 = set(dec.graphs)
    a7 = dec.generate(tb, zeroed(tb), length, 7.5, **kw)
    assert keys3 and all(("guidance", 3.0) in k for k in keys3)
    new = set(dec.graphs) - keys3
    assert new and all(("guidance", 7.5) in k for k in new) and len(new) == len(keys3)
    for s, got in ((3.0, a3), (7.5, a7)):
        assert torch.equal(got, GuidedDecoder(model, 3, max_len=length).generate(tb, zeroed(tb), length, s, **kw))
    same = [dec.generate(tb, tb, length, s, **kw) for s in (1.0, 3.0, 7.5)]          # negative == prompt: lu at any scale
    assert torch.equal(same[0], same[1]) and torch.equal(same[0], same[2])
    perm = [2, 0, 1]
    take = lambda b: {k: v[perm] for k, v in b.items()}
    assert torch.equal(dec.generate(take(tb), take(zeroed(tb)), length, 3.0, **kw), a3[perm])
    # a plain decoder keeps the graph keys it had
    plain = GreedyDecoder(model, 3, max_len=length)
    plain.generate(tb, length, **kw)
    assert not any(any(isinstance(e, tuple) and e and e[0] == "guidance" for e in k) for k in plain.graphs)


# ------------------------------------------------------------------ 6. the surface
class Tok:
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    def convert_ids_to_tokens(self, ids):
        return [self.names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

    def convert_tokens_to_ids(self, t):
        return {"[#START#]": 1, "[#EOS#]": 2, "[UNK]": 100, "[SEP]": 102}[t]


def test_generate_samples_takes_the_arguments_and_scale_one_is_the_call_without_them():
    from mmtg_amd.generate import generate_samples
    model, tb = tiny("f32")
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    gen = lambda: torch.Generator(device=DEV).manual_seed(4)
    kw = dict(n_samples=2, length=2 * SENT, line_lengths=7)
    texts = generate_samples(model, rows, Tok(), generator=gen(), guidance_scale=3.0, **kw)
    assert len(texts) == 3 and all(len(t) == 2 and all(isinstance(x, str) and x for x in t) for t in texts)
    assert texts == generate_samples(model, rows, Tok(), generator=gen(), guidance_scale=3.0, **kw)
    for t in texts:                                                              # seven characters a line
        assert all(len(x.split("，")[0]) == 7 for x in t)
    plain = generate_samples(model, rows, Tok(), generator=gen(), **kw)
    assert plain != texts
    assert generate_samples(model, rows, Tok(), generator=gen(), guidance_scale=3.0, negative_rows={k: v[:1] for k, v in rows.items()},
                            **kw) != texts                                       # one negative for all: another steer
    ranked = generate_samples(model, rows, Tok(), generator=gen(), guidance_scale=3.0, rank_by="mean", **kw)
    for t, r in zip(texts, ranked):
        assert sorted(t) == sorted(x for x, _, _ in r)
        means = [lp / max(cnt, 1) for _, lp, cnt in r]
        assert means == sorted(means, reverse=True) and all(np.isfinite(m) and m < 0 for m in means)
    # scale 1 is the plain call: the same ids, the same decoder, no guided graph key
    dec = GreedyDecoder(model, 6, max_len=2 * SENT)
    a = generate_samples(model, rows, Tok(), generator=gen(), decoder=dec, **kw)
    keys = set(dec.graphs)
    b = generate_samples(model, rows, Tok(), generator=gen(), decoder=dec, guidance_scale=1.0, **kw)
    assert a == b == plain and set(dec.graphs) == keys


def test_scores_under_guidance_are_the_models_own_and_mirostat_moves_the_prompts_rows_only():
    from mmtg_amd.generate import score_sequences
    model, tb = tiny("f32")
    length = 2 * SENT
    dec = GuidedDecoder(model, 3, max_len=length)
    gen = torch.Generator(device=DEV).manual_seed(9)
    ids, lp = dec.generate(tb, zeroed(tb), length, 3.0, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0, mirostat_tau=2.0,
                           generator=gen, return_logprobs=True)
    mu = dec.mirostat_mu.cpu()
    assert bool((mu[3:] == 4.0).all()) and bool((mu[:3] != 4.0).all())
    assert lp.shape == ids.shape and bool((dec.tok_lp[3:] == 0).all())
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    want = score_sequences(model, rows, ids)
    np.testing.assert_allclose(lp.cpu().numpy(), want, atol=ATOL, rtol=0)          # (test_logprob_gpu.py's tolerance)
    assert float(np.abs(want).sum()) > 0


def test_sample_sequence_with_guidance_is_the_one_prompt_guided_decoder():
    from mmtg_amd.generate import sample_sequence
    model, tb = tiny("f32")
    length = 2 * SENT
    start = {k: v[0].cpu().numpy() for k, v in tb.items()}
    start["targets"] = np.asarray([1])
    got = sample_sequence(model, start, length, Tok(), temperature=T, top_k=1, top_p=0.0, repitition_penalty=REP, guidance_scale=3.0)
    one = {k: v[:1] for k, v in tb.items()}
    ids = GuidedDecoder(model, 1, max_len=length).generate(one, zeroed(one), length, 3.0, temperature=T, repitition_penalty=REP)
    assert got == GreedyDecoder.reference_return(ids[0].tolist(), length)
    assert got != sample_sequence(model, start, length, Tok(), temperature=T, top_k=1, top_p=0.0, repitition_penalty=REP)


@pytest.mark.parametrize("row", [0, 1, 2])
def test_the_rerun_loop_with_guidance_agrees_with_the_cached_path_up_to_the_first_near_tie(monkeypatch, row):
    """MMTG_SAMPLE_RERUN=1 runs sample_sequence's prefix re-run loop: two forwards per token and mmtg_decode_guidance on the two last
    rows.  In f32 its ids are the cached path's up to the first step whose float64 top-2 margin of the processed guided scores is under
    1e-3 (set aside as in the host-loop test: the two paths' logits differ in the last bits).  Each prompt of the fixture in turn."""
    from mmtg_amd.generate import sample_sequence
    model, tb = tiny("f32")
    length, s = 2 * SENT, 3.0
    start = {k: v[row].cpu().numpy() for k, v in tb.items()}
    start["targets"] = np.asarray([1])
    kw = dict(temperature=T, top_k=1, top_p=0.0, repitition_penalty=REP, guidance_scale=s)
    cached = sample_sequence(model, start, length, Tok(), **kw)
    one = {k: v[row:row + 1] for k, v in tb.items()}
    dec = GuidedDecoder(model, 1, max_len=length)
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    ties = []

    def tap(j, with_head, picked, logits):
        if with_head and int(dec.seq[0, P + j - 1]) != 0:
            g = torch.from_numpy(guidance_scores(logits[0, :V].double().cpu().numpy(), logits[1, :V].double().cpu().numpy(), s))
            top = torch.sort(O.process_logits(g, dec.seq[0, P:P + j].cpu(), T, REP), descending=True).values
            if float(top[0] - top[1]) < 1e-3:
                ties.append(j)

    ids = dec.generate(one, zeroed(one), length, s, temperature=T, repitition_penalty=REP, tap=tap)
    assert cached == GreedyDecoder.reference_return(ids[0].tolist(), length)
    monkeypatch.setenv("MMTG_SAMPLE_RERUN", "1")
    rerun = sample_sequence(model, start, length, Tok(), **kw)
    upto = min(ties) if ties else len(cached)
    print("re-run loop, prompt %d: %d ids, near-ties at columns %s, compared up to %d" % (row, len(rerun), ties, upto))
    assert len(rerun) == len(cached) and upto > 1 and rerun[:upto] == cached[:upto]
    plain = sample_sequence(model, start, length, Tok(), **dict(kw, guidance_scale=1.0))
    assert plain != rerun                                                        # the guided branch ran
    neg = {k: (np.zeros_like(v) if k in ("img_embs", "r_embs") else v) for k, v in start.items()}
    assert sample_sequence(model, start, length, Tok(), negative_input=neg, **kw) == rerun      # the default negative, given


def test_generate_samples_scores_under_guidance_are_score_sequences_of_its_own_ids():
    """generate_samples(..., guidance_scale=3, return_scores=True): each sample's sum is sequence_scores of what score_sequences -- the
    plain decoder, teacher-forced, knowing nothing of guidance -- gives the sample's own ids under its real prompt."""
    from mmtg_amd.constraints import sequence_scores
    from mmtg_amd.generate import generate_samples, score_sequences
    model, tb = tiny("f32")
    length, k = 2 * SENT, 2
    rows = {key: v.cpu().numpy() for key, v in tb.items()}
    dec = GuidedDecoder(model, 3 * k, max_len=length)
    scored = generate_samples(model, rows, Tok(), n_samples=k, length=length, guidance_scale=3.0, return_scores=True, decoder=dec,
                              generator=torch.Generator(device=DEV).manual_seed(6))
    P = dec.eng.sh.P
    ids = dec.seq[:3 * k, P:P + 1 + length].cpu()                                # the one chunk's rows: prompt r // k, sample r % k
    lp = score_sequences(model, {key: np.repeat(v, k, 0) for key, v in rows.items()}, ids)
    upto = len(GreedyDecoder.reference_return(ids[0].tolist(), length))
    sums, counts = sequence_scores(ids.numpy(), lp, sent=SENT, upto=upto)
    flat = [e for prompt in scored for e in prompt]
    assert len(flat) == 3 * k and dec.graphs
    for r, (text, total, cnt) in enumerate(flat):
        assert isinstance(text, str) and text
        assert cnt == int(counts[r]) and cnt > 10 and abs(total - float(sums[r])) <= ATOL * cnt, (r, total, float(sums[r]))
