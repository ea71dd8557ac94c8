"""Contrastive search (mmtg_amd.decode.ContrastiveDecoder) on the MI355X: the similarity kernel against float64, the merge kernel
against a numpy restatement of include/mmtg_hip.h, alpha = 0 and top_k = 1 against the greedy decoder, the decoder against the CPU
contrastive search of tests/test_contrastive_cpu.py, a held prefix, determinism at full size and the text surface."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_case  # noqa: E402
from mmtg_amd import hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, ContrastiveDecoder, GreedyDecoder  # noqa: E402
from test_beam_cpu import SENT, setup_case, start_row  # noqa: E402
from test_beam_gpu import build, full_size_model  # noqa: E402
from test_contrastive_cpu import FOLLOW, REP, T, comparable, cpu_contrastive_search, follow_runs, truncate  # noqa: E402

DEV = "cuda"
NEG = float("-inf")


# ------------------------------------------------------------------ 1. the similarity kernel against float64
CTX = (0, 1, 7, 8, 9, 63, 64, 65, 236)      # 8 columns per pass of a workgroup (4 waves x 2): 7 / 8 / 9 are its chunk size -+ 1
TINY_D = load_case("tiny_s5")[3]["n_embd"]


def _unit_ln_f64(x, gamma, beta, eps):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    h = (xd - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    n = torch.sqrt((h * h).sum(1, keepdim=True))
    return torch.where(n > 0, h / n, torch.zeros_like(h))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", sorted({TINY_D, 768, 1024}))
def test_similarity_kernel_against_float64(D, dtype):
    """Per row: hc[b, pos - P] within D * 2^-23 of the float64 unit(ln_f(x)) elementwise, sim within 2 * D * 2^-24 of the float64
    maximum over the STORED fp32 unit vectors (the worst-case fp32 dot-product bound for unit vectors), exactly 0 for an empty
    context, nothing else of the cache touched.  A random (non-identity) ancestry table, zeros in keep inside the context, a row
    whose context is all PAD, a dead row; 2 prompts x k in {1, 4, 16}; context lengths around the kernel's pass of 8 columns, the
    wave count and the full lyric."""
    P, HC, eps = 5, 240, 1e-5
    Tmax = P + HC + 1
    worst_u = worst_s = 0.0
    for k in (1, 4, 16):
        B = 2 * k
        g = torch.Generator().manual_seed(100 * k + D)
        hc0 = torch.randn(B, HC, D, generator=g)
        hc0 = (hc0 / hc0.norm(dim=2, keepdim=True)).contiguous()
        keep = (torch.rand(B, Tmax, generator=g) > 0.25).to(torch.int32)
        rows = torch.randint(0, B, (B, Tmax), generator=g, dtype=torch.int32)
        assert not torch.equal(rows, torch.arange(B, dtype=torch.int32)[:, None].expand(B, Tmax)) or B == 1
        x = (torch.randn(B, D, generator=g) * 2 + 0.5).to(dtype)
        gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
        scores = -torch.rand(B, generator=g)
        dead = B - 1
        scores[dead] = NEG
        blank = B - 2 if B >= 4 else None           # a row whose lyric so far is PAD throughout
        if blank is not None:
            keep[blank, P:] = 0
        want_u = _unit_ln_f64(x, gamma, beta, eps)
        d = [t.to(DEV) for t in (x, gamma, beta, keep, rows, scores)]
        for c in CTX:
            hc = hc0.clone().to(DEV)
            sim = torch.full((B,), 7.0, device=DEV)
            posd = torch.tensor([P + c], dtype=torch.int32, device=DEV)
            hip.decode_contrastive_sim(d[0], d[1], d[2], eps, hc, sim, d[3], d[4], posd, P, B, D, scores=d[5])
            torch.cuda.synchronize()
            hc, sim = hc.cpu(), sim.cpu()
            got_u = hc[:, c].clone()
            err_u = float((got_u.double() - want_u).abs().max())
            worst_u = max(worst_u, err_u)
            assert err_u <= D * 2.0 ** -23, (k, c, err_u)
            hc[:, c] = hc0[:, c]
            assert torch.equal(hc, hc0), (k, c)
            for b in range(B):
                ts = [t for t in range(c) if int(keep[b, P + t])]
                if b == dead or not ts:
                    assert float(sim[b]) == 0.0, (k, c, b)
                    continue
                ctx = hc0[rows[b, P + torch.tensor(ts)].long(), torch.tensor(ts)].double()
                want = float((ctx @ got_u[b].double()).max())
                worst_s = max(worst_s, abs(float(sim[b]) - want))
                assert abs(float(sim[b]) - want) <= 2 * D * 2.0 ** -24, (k, c, b, float(sim[b]), want)
            if blank is not None:
                assert float(sim[blank]) == 0.0
    # without scores every row is read; inside the prompt nothing is written
    hc = hc0.clone().to(DEV)
    sim = torch.full((B,), 7.0, device=DEV)
    hip.decode_contrastive_sim(d[0], d[1], d[2], eps, hc, sim, d[3], d[4], torch.tensor([P + 9], dtype=torch.int32, device=DEV), P, B, D)
    assert float(sim[dead]) != 0.0 and float(sim[dead]) != 7.0
    hip.decode_contrastive_sim(d[0], d[1], d[2], eps, hc, sim, d[3], d[4], torch.tensor([P - 1], dtype=torch.int32, device=DEV), P, B, D)
    torch.cuda.synchronize()
    hc = hc.cpu()
    hc[:, 9] = hc0[:, 9]
    assert torch.equal(hc, hc0)
    print("similarity D=%d %s: max |u - u64| %.3e (bound %.3e), max |sim - sim64| %.3e (bound %.3e)"
          % (D, str(dtype).split(".")[-1], worst_u, D * 2.0 ** -23, worst_s, 2 * D * 2.0 ** -24))


def test_similarity_kernel_past_its_cache_penalises_nothing():
    """A position the hidden cache has no column for: nothing is stored or read, and sim is 0 rather than the step before's."""
    P, B, D = 5, 8, 768
    g = torch.Generator().manual_seed(3)
    hc0 = torch.randn(B, 8, D, generator=g)
    hc, sim = hc0.clone().to(DEV), torch.full((B,), 7.0, device=DEV)
    x, gamma, beta = torch.randn(B, D, generator=g).to(DEV), torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    keep = torch.ones(B, 32, dtype=torch.int32, device=DEV)
    rows = torch.arange(B, dtype=torch.int32, device=DEV)[:, None].expand(B, 32).contiguous()
    hip.decode_contrastive_sim(x, gamma, beta, 1e-5, hc, sim, keep, rows, torch.tensor([P + 8], dtype=torch.int32, device=DEV), P, B, D)
    torch.cuda.synchronize()
    assert torch.equal(hc.cpu(), hc0) and (sim == 0).all()


# ------------------------------------------------------------------ 2. the merge kernel against a numpy restatement
def merge_reference(cv, ci, scores, sim, total, alpha, seq, keep, rows, pos, P, k, fixed_end):
    """The merge rule of include/mmtg_hip.h on host copies; returns (seq, keep, rows, scores, total, the chosen r* per prompt)."""
    seq, keep, rows, scores, total = seq.copy(), keep.copy(), rows.copy(), scores.copy(), total.copy()
    B = seq.shape[0]
    j = pos + 1 - P
    if pos < P:
        rows[:, pos + 1] = np.arange(B)
        return seq, keep, rows, scores, total, None
    chosen = []
    a = np.float32(alpha)
    for g_ in range(B // k):
        b0 = g_ * k
        best, rs = None, 0
        for r in range(k):
            s = scores[b0 + r]
            if not s > -np.inf:
                continue
            cs = np.float32(np.float32(1.0) - a) * np.exp(s, dtype=np.float32) - a * sim[b0 + r]
            if best is None or cs > best:
                best, rs = cs, r
        chosen.append(rs)
        bs = b0 + rs
        for t in (seq, keep, rows):
            t[b0:b0 + k, pos] = t[bs, pos]
        total[g_] = np.float32(total[g_] + scores[bs])
        new = np.full(k, -np.inf, np.float32)
        new[0] = 0.0
        if fixed_end is not None and pos + 1 < fixed_end[b0]:
            pass
        elif j > 1 and (j + 1) % SENT in (0, 1):
            seq[b0:b0 + k, pos + 1] = 2 if (j + 1) % SENT == 0 else 1
        elif cv is not None:
            seq[b0:b0 + k, pos + 1] = ci[bs]
            new = cv[bs].copy()
        scores[b0:b0 + k] = new
        rows[b0:b0 + k, pos + 1] = np.arange(b0, b0 + k)
    return seq, keep, rows, scores, total, chosen


def _merge_inputs(k, alphas, P, Tmax):
    """Five prompts: r* = 0, r* = the last row, an exact tie of two rows (the lower wins), a dead row with the best similarity, a
    prompt at its start state [0, -inf, ...].  Every other pair of contrastive scores of a prompt differs by 1e-3 or more at every
    alpha used (drawn again until it does), so fp32 rounding decides nothing."""
    n = 5
    B = n * k
    for seed in range(200):
        g = np.random.default_rng(1000 * k + seed)
        p = g.uniform(0.05, 0.95, B)
        sim = g.uniform(0.0, 0.9, B)
        if k >= 4:
            p[0], sim[0] = 0.99, -0.5                                   # prompt 0: row 0
            p[2 * k - 1], sim[2 * k - 1] = 0.99, -0.5                   # prompt 1: the last row
            p[2 * k + 1], sim[2 * k + 1] = 0.99, -0.5                   # prompt 2: rows 1 and 2 tie
            p[2 * k + 2], sim[2 * k + 2] = 0.99, -0.5
            p[3 * k + 2], sim[3 * k + 2] = 0.0, -0.9                    # prompt 3: a dead row with the best similarity
        p[4 * k + 1:5 * k] = 0.0                                        # prompt 4: the start state
        p[4 * k] = 1.0
        ok = True
        for a in alphas:
            cs = (1 - a) * p - a * sim
            for g_ in range(n):
                v = np.sort([cs[g_ * k + r] for r in range(k) if p[g_ * k + r] > 0])
                d = np.diff(v)
                ok = ok and bool(np.all((d >= 1e-3) | (d == 0))) and int((d == 0).sum()) == (1 if (g_ == 2 and k >= 4) else 0)
        if ok:
            break
    assert ok
    with np.errstate(divide="ignore"):
        scores = np.log(p).astype(np.float32)
    t = torch.Generator().manual_seed(k)
    seq = torch.randint(30, 99, (B, Tmax), generator=t).numpy()
    keep = torch.randint(0, 2, (B, Tmax), generator=t, dtype=torch.int32).numpy()
    rows = torch.randint(0, B, (B, Tmax), generator=t, dtype=torch.int32).numpy()
    cv = -torch.rand(B, k, generator=t).numpy().astype(np.float32) * 4
    cv[:, k - 1:] = -np.inf if k > 1 else cv[:, k - 1:]                 # (a filler candidate, as the candidates kernel writes it)
    ci = torch.randint(3, 160, (B, k), generator=t, dtype=torch.int32).numpy()
    total = -torch.rand(n, generator=t).numpy().astype(np.float32) * 30
    return scores, sim.astype(np.float32), seq, keep, rows, cv, ci, total


@pytest.mark.parametrize("k", [1, 4, 16])
def test_merge_kernel_against_the_numpy_restatement(k):
    """Integers exact, floats bit-equal (copies, or one fp32 add): column pos of seq / keep / rows on every row, column pos + 1,
    scores, total, rows[:, pos + 1] and the published position -- at a column with candidates, the forced [#EOS#] and [#START#]
    columns, held prefix columns (some prompts held, some past their prefix, one exactly at its end), null candidates and inside
    the prompt; alpha 0.6, 0 and 1."""
    P, Tmax, n = 5, 64, 5
    B = n * k
    alphas = (0.6, 0.0, 1.0)
    scores, sim, seq, keep, rows, cv, ci, total = _merge_inputs(k, alphas, P, Tmax)
    fe = np.repeat(np.array([P + 15, P + 5, P + 11, P + 30, P + 1], np.int32), k)       # at pos = P + 10: held, past, at the end, held, past
    runs = [(P + 10, True, None), (P + 20, True, None), (P + 21, True, None), (P + 42, True, None), (P + 10, True, fe),
            (P + 20, True, fe), (P + 10, False, None), (P + 10, False, fe), (P - 2, True, None), (P, True, None), (Tmax - 2, True, None)]
    for alpha in alphas:
        for pos, with_cand, fixed in runs:
            d = [torch.from_numpy(t.copy()).to(DEV) for t in (scores, sim, total, seq, keep, rows, cv, ci)]
            dsc, dsim, dtot, dseq, dkeep, drows, dcv, dci = d
            posd = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
            hip.decode_contrastive_merge(dcv if with_cand else None, dci if with_cand else None, dsc, dsim, dtot, alpha, dseq, dkeep, drows,
                                         posd[0:1], P, SENT, k, n, pos_next=posd[1:2],
                                         fixed_end=None if fixed is None else torch.from_numpy(fixed).to(DEV))
            torch.cuda.synchronize()
            rseq, rkeep, rrows, rsc, rtot, chosen = merge_reference(cv if with_cand else None, ci, scores, sim, total, alpha, seq, keep,
                                                                    rows, pos, P, k, fixed)
            what = (alpha, pos, with_cand, fixed is not None)
            assert int(posd[1]) == pos + 1 and int(posd[0]) == pos, what
            assert np.array_equal(dseq.cpu().numpy(), rseq) and np.array_equal(dkeep.cpu().numpy(), rkeep), what
            assert np.array_equal(drows.cpu().numpy(), rrows), what
            assert np.array_equal(dsc.cpu().numpy().view(np.int32), rsc.view(np.int32)), what
            assert np.array_equal(dtot.cpu().numpy().view(np.int32), rtot.view(np.int32)), what
            if chosen is not None and k >= 4 and 0 < alpha:
                assert chosen[:3] == [0, k - 1, 1] and chosen[3] != 2 and chosen[4] == 0, (what, chosen)


# ------------------------------------------------------------------ 3. alpha = 0 and top_k = 1 are the greedy decoder
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", ["tiny_s5", "full_12l"])
def test_without_a_penalty_or_a_choice_it_is_the_greedy_decoder(case, mode):
    model, tb = build(case, mode)
    n = tb["img_embs"].shape[0]
    length = 220
    kw = dict(temperature=T, repitition_penalty=REP)
    rules = dict(no_repeat_ngram_size=3, line_lengths=(1, 20))
    g = GreedyDecoder(model, n)
    greedy, ruled = g.generate(tb, length, **kw), g.generate(tb, length, **kw, **rules)
    dec = ContrastiveDecoder(model, n, 4)
    assert dec.x3 == (mode == "bf16x3") and (mode != "bf16" or dec.fused)
    ids, scores = dec.generate(tb, length, penalty_alpha=0.0, **kw)
    assert tuple(ids.shape) == (n, 1 + length) and tuple(scores.shape) == (n,)
    assert torch.equal(ids, greedy)
    _, one = BeamDecoder(model, n, 1).generate(tb, length, **kw)
    np.testing.assert_allclose(scores.cpu().numpy(), one[:, 0].cpu().numpy(), rtol=0, atol=1e-3)
    ids, _ = dec.generate(tb, length, penalty_alpha=0.0, **kw, **rules)            # a constrained candidates form in the path
    assert torch.equal(ids, ruled)
    ids, s1 = ContrastiveDecoder(model, n, 1).generate(tb, length, penalty_alpha=0.6, **kw)
    assert torch.equal(ids, greedy)
    np.testing.assert_allclose(s1.cpu().numpy(), one[:, 0].cpu().numpy(), rtol=0, atol=1e-3)
    keys = list(dec.graphs)
    assert keys and all(("contrastive", 0.0) in key_ for key_ in keys)


# ------------------------------------------------------------------ 4. the decoder follows the CPU search
def _rows_agree(dec, L):
    """The invariant: at the end of a run the k rows of a prompt hold the same ids in every column but the last."""
    P = dec.eng.sh.P
    s = dec.seq[:, P:P + L].reshape(dec.n_prompts, dec.nb, L)
    return bool((s == s[:, :1]).all())


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", sorted(FOLLOW))
def test_it_follows_the_cpu_contrastive_search(case, mode):
    """Every prompt is compared over the generation length before its first CPU choice made by less than 1e-4 (there two fp32
    searches may choose differently): ids equal, scores within 1e-3.  The CPU test holds the fixtures to at least 40 such
    columns on some prompt and at least 3 choices of a candidate other than the most probable one inside them."""
    k, alpha, full = FOLLOW[case]
    recs = follow_runs(case)
    lens = [comparable(rec, full) for rec in recs]
    assert max(lens) >= 40 and sum(sum(1 for e in rec[:L] if e["r"] != 0) for rec, L in zip(recs, lens)) >= 3, lens
    model, tb = build(case, mode)
    n = tb["img_embs"].shape[0]
    dec = ContrastiveDecoder(model, n, k, max_len=full)
    runs = {}
    for row, L in enumerate(lens):
        if L < 1:
            continue
        if L not in runs:
            runs[L] = [t.cpu() for t in dec.generate(tb, L, penalty_alpha=alpha, temperature=T, repitition_penalty=REP)]
            assert _rows_agree(dec, L), (row, L)
        ids, scores = runs[L]
        cids, cscore = truncate(recs[row], L)
        assert ids[row].tolist() == cids, (row, L)
        assert abs(float(scores[row]) - float(cscore)) <= 1e-3, (row, L, float(scores[row]), float(cscore))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_the_step_scores_its_own_final_residual_stream(mode):
    """End to end, with the penalty on: after the last token step of a run, the cache column it wrote is unit(ln_f(dec.h)) of the
    residual stream the step left (bf16 in the fused bf16 step, fp32 in the split-precision one) within D * 2^-23 of float64, and
    dec.sim is the float64 maximum over the stored unit vectors of the row's kept lyric columns, read through the ancestry table,
    within 2 * D * 2^-24 -- 0 for a row that was dead when the step ran.  The similarity launch's bounds, on the decoder's own data."""
    model, tb = build("tiny_s5", mode)
    n, k, L = tb["img_embs"].shape[0], 4, 60
    dec = ContrastiveDecoder(model, n, k, max_len=L)
    assert dec.x3 == (mode == "bf16x3") and (mode != "bf16" or dec.fused)
    sh = dec.eng.sh
    P, D = sh.P, sh.D
    n_steps = dec.begin(tb, L, temperature=T, repitition_penalty=REP, penalty_alpha=0.6)
    for pos in range(dec.first_pos, n_steps - 1):
        dec.step_at(pos)
    before = dec.scores.cpu().clone()                       # which rows the last step's similarity launch sees alive
    dec.step_at(n_steps - 1)
    torch.cuda.synchronize()
    assert dec.h.dtype == (torch.bfloat16 if mode == "bf16" else torch.float32)
    pre = "decoder.gpt2.transformer."
    want_u = _unit_ln_f64(dec.h.cpu(), dec.eng.P(pre + "ln_f.weight").cpu(), dec.eng.P(pre + "ln_f.bias").cpu(), sh.eps)
    hc, sim, rows, keep = dec.Hc.cpu(), dec.sim.cpu(), dec.rows.cpu(), dec.keep.cpu()
    c = L - 1
    assert float((hc[:, c].double() - want_u).abs().max()) <= D * 2.0 ** -23
    alive = 0
    for b in range(n * k):
        if not float(before[b]) > NEG:
            assert float(sim[b]) == 0.0
            continue
        alive += 1
        ts = torch.tensor([t for t in range(c) if int(keep[b, P + t])])
        ctx = hc[rows[b, P + ts].long(), ts].double()
        assert abs(float(sim[b]) - float((ctx @ hc[b, c].double()).max())) <= 2 * D * 2.0 ** -24, b
    assert alive >= n and float(sim.abs().max()) > 0


# ------------------------------------------------------------------ 5. a prefix is held, and the search goes on from it
PRE = [1] + list(range(30, 37)) + [0] * 13 + [2] + [1] + list(range(40, 47)) + [0] * 13 + [2] + [1]      # two lines and the next [#START#]


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_a_given_opening_comes_back_and_the_continuation_follows_the_cpu_search(mode):
    """At the usual k = 4, alpha = 0.6: behind the 45 given ids the CPU search's comparable lengths are 63 / 67 / 100 of 100 (one
    choice of a candidate other than the most probable one on the last prompt)."""
    case, k, alpha, full = "tiny_s5", 4, 0.6, 100
    fx, sh, w, table, batch = setup_case(case)
    model, tb = build(case, mode)
    n = tb["img_embs"].shape[0]
    dec = ContrastiveDecoder(model, n, k, max_len=full)
    kw = dict(penalty_alpha=alpha, temperature=T, repitition_penalty=REP, prefix=[PRE] * n)
    ids, scores = dec.generate(tb, full, **kw)
    assert ids[:, :len(PRE)].cpu().tolist() == [PRE] * n and torch.isfinite(scores).all() and _rows_agree(dec, full)
    assert dec.first_pos == sh.P and any("prefix" in key_ for key_ in dec.graphs)     # every lyric column went through a token step
    lens = []
    for row in range(n):
        rec = cpu_contrastive_search(w, sh, table, start_row(batch, row), full, k, alpha, T, REP, prefix=PRE)
        L = comparable(rec, full)
        lens.append(L)
        if L < len(PRE):
            continue
        got, sc = dec.generate(tb, L, **kw)
        cids, cscore = truncate(rec, L)
        assert got[row].cpu().tolist() == cids, (row, L)
        assert abs(float(sc[row]) - float(cscore)) <= 1e-3, (row, L)
    assert max(lens) >= len(PRE) + 10, lens


# ------------------------------------------------------------------ 6. determinism at full size
def test_full_size_contrastive_runs_are_bit_stable():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    n, k, Ln = 64, 4, 220
    nbt = synth.make_batch(n, mcfg, dcfg, V, seed=11)
    batch = {k_: torch.from_numpy(np.asarray(v)).to(DEV) for k_, v in nbt.items() if k_ not in ("rating", "targets")}
    dec = ContrastiveDecoder(model, n, k, max_len=Ln)
    assert dec.fused and dec.use_graph
    i1, s1 = dec.generate(batch, Ln, penalty_alpha=0.6, temperature=T, repitition_penalty=REP)
    i2, s2 = dec.generate(batch, Ln, penalty_alpha=0.6, temperature=T, repitition_penalty=REP)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    assert _rows_agree(dec, Ln)
    assert torch.isfinite(s1).all() and (s1 < 0).all()
    assert int(i1.min()) >= 0 and int(i1.max()) < V and (i1[:, 0] == 1).all()
    greedy, _ = dec.generate(batch, Ln, penalty_alpha=0.0, temperature=T, repitition_penalty=REP)
    assert not torch.equal(greedy, i1)                      # the penalty changes the lyric


# ------------------------------------------------------------------ 7. the text surface
def test_generate_contrastive_texts_and_rhymes():
    from mmtg_amd.generate import encode_rhyme_classes, generate_contrastive
    from test_rhyme_cpu import fixture_rhymes
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

        def convert_tokens_to_ids(self, t):
            return ord(t) - 0x4e00 if 0x4e00 <= ord(t) < 0x4e00 + 160 else 100

    tok = Tok()
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    out = generate_contrastive(model, rows, tok, top_k=4, penalty_alpha=0.6, length=66)
    assert len(out) == 3
    for text, score in out:
        assert isinstance(text, str) and text and np.isfinite(score) and score < 0
    sets, bounds = fixture_rhymes(fx)
    classes = encode_rhyme_classes(tok, ["".join(chr(0x4e00 + v) for v in sorted(k_)) for k_ in sets], vocab_cut=160)
    which = lambda v: next((i for i, k_ in enumerate(classes) if v in k_), None)      # noqa: E731
    out = generate_contrastive(model, rows, tok, top_k=4, penalty_alpha=0.6, length=4 * SENT, line_lengths=bounds, rhyme_scheme="AABB",
                               rhyme_classes=classes, return_ids=True, max_batch=8)   # two prompts per chunk, the last one padded
    assert len(out) == 3
    for text, score, ids in out:
        assert np.isfinite(score) and score < 0 and len(ids) == 1 + 4 * SENT and len(text.split("，")) == 4
        ends = []
        for l in range(4):
            body = [v for v in ids[l * SENT + 1:l * SENT + SENT - 1] if v != 0]
            assert 3 <= len(body) <= 8, (l, body)
            ends.append(which(body[-1]))
        assert ends[0] is not None and ends[0] == ends[1] and ends[2] is not None and ends[2] == ends[3], (text, ends)
