"""Line-length bounds and line-end token sets on the MI355X: the *_lines selection entries against their plain / *_fixed / *_ngram
namesakes on logits the test has pre-banned, the decoders (GreedyDecoder / BeamDecoder with line_lengths= / line_end_ids=) against
the CPU restatements of tests/test_lines_cpu.py, sampling against a host restatement driven by the decoder's own uniforms, mixed
rows, prefixes, n-gram bans, off-means-off, full-size determinism and the text surface.  Every chosen column of every output row
is held to the rule (test_lines_cpu.rule_violations skips none)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmtg_amd import hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_lines  # noqa: E402
from mmtg_amd.generate import top_k_top_p_filtering  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case, start_row  # noqa: E402
from test_lines_cpu import (CAP, apply_rule, cpu_lines_beam_search, cpu_lines_greedy, end_sets_for, line_lengths_of, line_rule,  # noqa: E402
                            rule_violations)
from test_ngram_cpu import banned_ids  # noqa: E402
from test_ngram_gpu import _histories, build, full_size_model  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402

DEV = "cuda"


def device_tables(t):
    """check_lines' tables as the (lo, hi, sets, set_of) device tuple of the hip.decode_*_lines bindings."""
    up = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)      # noqa: E731
    return up(t.lo), up(t.hi), up(t.sets), up(t.set_of)


def all_violations(ids, tables, prefixes=None, n=0):
    """(row, columns) of every row of ids [B, 1 + length] that breaks the rule of its row of tables after its prefix."""
    ids = ids.cpu().tolist()
    out = []
    for b, r in enumerate(ids):
        v = rule_violations(r, tables, b, start=len(prefixes[b]) if prefixes else 1, n=n)
        if v:
            out.append((b, v))
    return out


# ------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("n", [0, 2, 3])
def test_lines_entries_equal_their_namesakes_on_pre_banned_logits(n):
    """Each *_lines entry writes bit for bit what its namesake (*_ngram for n > 0, else plain or *_fixed) writes on the same logits
    with the rule applied beforehand on the host: PAD at -inf where it is banned, every id outside the end set at -inf in the set's
    column, everything but PAD at -inf where the line is full (the namesake then picks PAD / offers PAD at log-probability 0).
    Covers sticky-PAD rows, forced columns, held prefix rows and a line past the tables."""
    B, P, V, Vp, Tmax, nb = 8, 5, 160, 168, 64, 4
    g = torch.Generator().manual_seed(300 + n)
    logits = torch.randn(B, Vp, generator=g) * 2
    logits[:, 3:6] += 6.0
    logits[:, 0] += 5.0                                                        # PAD is likely where it is allowed
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24).to(DEV)
    seq0 = _histories(B, P, Tmax, g)
    A, Bs = {3, 4}, {5, 40}
    lens = [[(4, 4), (0, 3)], [(0, 3), (5, 20)], [(5, 20), (0, 11)], [(0, 11), None], [None, (2, 9)], [(2, 9), (0, 9)],
            [(0, 9), (11, 11)], [(11, 11), (4, 4)]]
    ends = [[A, None], [None, None], [None, Bs], [Bs, None], [None, A], [None, A], [A, None], [None, A]]
    tabs = check_lines(lens, ends, B, 2 * SENT, SENT, V)                       # two lines: the third is past the tables
    dt = device_tables(tabs)
    kinds = {"full": 0, "pad": 0, "set": 0, "ngram": 0}
    for pos in (P + 3, P + 10, P + 20, P + 21, P + 25, P + 30, P + 47):        # c = 3, 10; [#EOS#]; [#START#]; line 1 c = 3, 8; line 2
        j = pos + 1 - P
        s0 = seq0.clone()
        s0[5, P + j - 1] = 0                                                  # a sticky-PAD row
        masked = logits.clone()
        if j % SENT not in (0, SENT - 1):
            for b in range(B):
                hist = s0[b, P:P + j].tolist()
                lo, hi, e = tabs.bounds(b, j // SENT)
                r = line_rule(hist, lo, hi, e)
                if hist[-1] == 0:
                    continue
                if r == "pad":
                    masked[b, 1:] = float("-inf")
                    kinds["full"] += 1
                    continue
                kinds["pad"] += r[0]
                kinds["set"] += r[1] is not None
                masked[b, :V] = apply_rule(logits[b, :V], hist, lo, hi, e)
                kinds["ngram"] += len(banned_ids(hist, n))
        s0, lg, mk = s0.to(DEV), logits.to(DEV), masked.to(DEV)
        for fe in (None, torch.tensor([0, pos + 2, 0, pos + 1, 0, 0, pos + 5, 0], dtype=torch.int32, device=DEV)):
            for kind in ("select", "sample"):
                a, b_ = s0.clone(), s0.clone()
                pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                if kind == "select":
                    if n:
                        hip.decode_select_ngram(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, B, n, fixed_end=fe, pos_next=pa[1:2])
                    elif fe is None:
                        hip.decode_select(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, B, pos_next=pa[1:2])
                    else:
                        hip.decode_select_fixed(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, B, fe, pos_next=pa[1:2])
                    hip.decode_select_lines(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, B, dt, ngram=n, fixed_end=fe, pos_next=pb[1:2])
                else:
                    if n:
                        hip.decode_sample_ngram(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, n, fixed_end=fe, pos_next=pa[1:2])
                    elif fe is None:
                        hip.decode_sample(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, pos_next=pa[1:2])
                    else:
                        hip.decode_sample_fixed(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, fe, pos_next=pa[1:2])
                    hip.decode_sample_lines(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, ngram=n, fixed_end=fe,
                                            pos_next=pb[1:2])
                torch.cuda.synchronize()
                assert int(pb[1]) == pos + 1 == int(pa[1])
                assert torch.equal(a, b_), (pos, kind, fe is None, a[:, pos + 1].tolist(), b_[:, pos + 1].tolist())
            cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
            cvb, cib = cva.clone(), cia.clone()
            pp = torch.tensor([pos], dtype=torch.int32, device=DEV)
            if n:
                hip.decode_beam_candidates_ngram(mk, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B, n, fixed_end=fe)
            elif fe is None:
                hip.decode_beam_candidates(mk, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B)
            else:
                hip.decode_beam_candidates_fixed(mk, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B, fe)
            hip.decode_beam_candidates_lines(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cvb, cib, B, dt, ngram=n, fixed_end=fe)
            torch.cuda.synchronize()
            assert torch.equal(cva, cvb) and torch.equal(cia, cib), (pos, fe is None)
    assert kinds["full"] > 0 and kinds["pad"] > 0 and kinds["set"] > 0 and (n == 0 or kinds["ngram"] > 0), kinds


def test_unconstrained_tables_through_the_lines_entries_are_the_plain_entries():
    B, P, V, Vp, Tmax, nb = 8, 5, 160, 168, 64, 4
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(B, Vp, generator=g) * 2).to(DEV)
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24).to(DEV)
    seq0 = _histories(B, P, Tmax, g).to(DEV)
    for tabs in (check_lines([None], None, B, 2 * SENT, SENT, V), check_lines((0, CAP), None, B, 2 * SENT, SENT, V)):
        dt = device_tables(tabs)
        for pos in (P, P + 7, P + 20, P + 21, P + 30):
            a, b_, c_, d_ = (seq0.clone() for _ in range(4))
            pp = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
            hip.decode_select(logits, Vp, V, a, pp[0:1], P, SENT, T, REP, B, pos_next=pp[1:2])
            hip.decode_select_lines(logits, Vp, V, b_, pp[0:1], P, SENT, T, REP, B, dt, pos_next=pp[1:2])
            hip.decode_sample(logits, Vp, V, c_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, pos_next=pp[1:2])
            hip.decode_sample_lines(logits, Vp, V, d_, pp[0:1], P, SENT, T, REP, 10, 0.7, uni, B, dt, pos_next=pp[1:2])
            cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
            cvb, cib = cva.clone(), cia.clone()
            hip.decode_beam_candidates(logits, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cva, cia, B)
            hip.decode_beam_candidates_lines(logits, Vp, V, seq0, pp[0:1], P, SENT, T, REP, nb, cvb, cib, B, dt)
            torch.cuda.synchronize()
            assert torch.equal(a, b_) and torch.equal(c_, d_) and torch.equal(cva, cvb) and torch.equal(cia, cib), pos


# ------------------------------------------------------------------ 2. decoders against the CPU restatements
def mixed_tables(fx, rows, length, V=160):
    """Different constraints per row: seven-token lines; no empty lines with end sets on every second line; a mix."""
    a, b_ = end_sets_for(fx, V)
    lens = [7, [(1, CAP), (1, 9), (1, CAP), (2, 6), (1, CAP), (3, 3)], [(2, 9), (0, 5), 5, None, (1, 6), (0, 2)]]
    ends = [None, [None, a, None, b_, None, a], [b_, None, a]]
    return check_lines(lens[:rows], ends[:rows], rows, length, SENT, V)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_greedy_under_the_rule_is_the_cpu_restatement(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    length = 6 * SENT
    tabs = mixed_tables(fx, 3, length)
    dec = GreedyDecoder(model, 3, max_len=220)
    plain = dec.generate(tb, length, temperature=T, repitition_penalty=REP).cpu()
    assert len(all_violations(plain, tabs)) == 3                               # the unconstrained run breaks the bounds it then gets
    for n in (0, 3):
        ids = dec.generate(tb, length, temperature=T, repitition_penalty=REP, line_lengths=tabs, no_repeat_ngram_size=n).cpu()
        assert all_violations(ids, tabs, n=n) == []
        assert line_lengths_of(ids[0].tolist()) == [7] * 6
        for row in range(3):
            want = cpu_lines_greedy(w, sh, table, start_row(batch, row), length, tabs, b=row, n=n)
            assert ids[row].tolist() == want, (n, row)
        got = line_lengths_of(ids[1].tolist())
        for l in (1, 3, 5):
            assert ids[1, l * SENT + got[l]].item() in tabs.bounds(1, l)[2]
    assert any("lines" in k for k in dec.graphs)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_four_beams_under_the_rule_follow_the_cpu_beam_search(mode):
    nb, full = 4, 6 * SENT
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    tabs = mixed_tables(fx, 3, full)
    lens = []
    for row in range(3):
        _, _, gaps = cpu_lines_beam_search(w, sh, table, start_row(batch, row), full, nb, tabs, b=row)
        lens.append(comparable_length(gaps, full))
    assert max(lens) >= 40, lens
    dec = BeamDecoder(model, 3, nb, max_len=full)
    runs = {}
    for row, L in enumerate(lens):
        if L < 1:
            continue
        if L not in runs:
            sub = check_lines([[tabs.bounds(b, l)[:2] for l in range((L - 1) // SENT + 1)] for b in range(3)],
                              [[tabs.bounds(b, l)[2] for l in range((L - 1) // SENT + 1)] for b in range(3)], 3, L, SENT, 160)
            runs[L] = [t.cpu() for t in dec.generate(tb, L, temperature=T, repitition_penalty=REP, line_lengths=sub)]
        ids, scores = runs[L]
        cids, cscores, _ = cpu_lines_beam_search(w, sh, table, start_row(batch, row), L, nb, tabs, b=row)
        assert ids[row].tolist() == cids.tolist(), (row, L)
        np.testing.assert_allclose(scores[row].numpy(), cscores, rtol=0, atol=1e-3)
        for k in range(nb):
            assert rule_violations(ids[row, k].tolist(), tabs, row) == []


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_one_beam_under_the_rule_is_greedy_under_the_rule(mode):
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", mode)
    tabs = mixed_tables(fx, 3, 220)
    for n in (0, 2):
        kw = dict(temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, line_lengths=tabs)
        greedy = GreedyDecoder(model, 3).generate(tb, 220, **kw)
        ids, scores = BeamDecoder(model, 3, 1).generate(tb, 220, **kw)
        assert torch.equal(ids[:, 0], greedy), n
        assert torch.isfinite(scores).all() and all_violations(greedy, tabs, n=n) == []
    # the raw forms: per prompt, shared by a prompt's beams
    a, _ = end_sets_for(fx)
    ids, _ = BeamDecoder(model, 3, 4).generate(tb, 220, temperature=T, repitition_penalty=REP, line_lengths=[[5] * 10, None, [(1, 3)] * 10],
                                               line_end_ids=[None, a])
    per = check_lines([[5] * 10, None, [(1, 3)] * 10], [None, a], 3, 220, SENT, 160)
    for b in range(3):
        for k in range(4):
            assert rule_violations(ids[b, k].tolist(), per, b) == []
    assert line_lengths_of(ids[0, 3].tolist()) == [5] * 10


def test_sampling_under_the_rule_follows_the_host_restatement_with_the_same_uniforms():
    """At every step that calls the head, each row's pick is the inverse-CDF draw (ids in index order, the decoder's own uniform of
    that position and row) from the step's logits processed on the host: penalty / temperature / fixed bans (the oracle's
    process_logits), the n-gram bans, the line rule, then the reference's top-k / top-p filter.  The draw is held to the fp32
    rounding of the CDF: u Z within 1e-4 Z of the pick's interval (160 terms of fp32 exp and sum err below 1e-5 Z)."""
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "f32")
    length, n, top_k, top_p = 6 * SENT, 3, 10, 0.7
    tabs = mixed_tables(fx, 3, length)
    dec = GreedyDecoder(model, 3, max_len=length)
    P, V = dec.eng.sh.P, min(dec.eng.sh.V, 13317)
    steps = []

    def tap(j, with_head, picked, logits):
        if with_head:
            steps.append((j, picked.cpu().tolist(), logits[:, :V].float().cpu().clone(), dec.seq[:, P:P + j].cpu().tolist(),
                          dec.uniforms[P + j - 1].cpu().tolist()))

    ids = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=top_k, top_p=top_p, no_repeat_ngram_size=n,
                       generator=torch.Generator(device=DEV).manual_seed(11), line_lengths=tabs, tap=tap).cpu()
    assert all_violations(ids, tabs, n=n) == []
    assert line_lengths_of(ids[0].tolist()) == [7] * 6
    checked = 0
    for j, picked, logits, hist, us in steps:
        for b in range(3):
            g = hist[b]
            if g[-1] == 0:
                assert picked[b] == 0
                continue
            lo, hi, e = tabs.bounds(b, j // SENT)
            x = O.process_logits(logits[b], torch.tensor(g), T, REP).clone()
            for v in banned_ids(g, n):
                x[v] = float("-inf")
            x = apply_rule(x, g, lo, hi, e)
            if x is None:
                assert picked[b] == 0
                continue
            if not torch.isfinite(x).any():
                assert picked[b] == 0
                continue
            f = top_k_top_p_filtering(x.clone(), top_k=top_k, top_p=top_p)
            assert torch.isfinite(f[picked[b]]), (j, b, picked[b])
            p = torch.exp(f.double() - f.double().max())
            cdf = torch.cumsum(p, 0)
            Z, target = float(cdf[-1]), us[b] * float(cdf[-1])
            assert float(cdf[picked[b]] - p[picked[b]]) - 1e-4 * Z <= target <= float(cdf[picked[b]]) + 1e-4 * Z, (j, b)
            checked += 1
    assert checked > 100
    again = dec.generate(tb, length, temperature=T, repitition_penalty=REP, top_k=top_k, top_p=top_p, no_repeat_ngram_size=n,
                         generator=torch.Generator(device=DEV).manual_seed(11), line_lengths=tabs).cpu()
    assert torch.equal(ids, again)


# ------------------------------------------------------------------ 3. prefixes, n-gram bans, mixed rows
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_partial_line_prefixes_continue_under_their_lines_bounds(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    a, b_ = end_sets_for(fx)
    line = batch["targets"][0, :SENT].tolist()
    pre = [batch["targets"][0, :SENT + 1].tolist() + line[1:4], line[:3], [1]]     # a whole line + 3 tokens; 2 tokens; none
    length = 4 * SENT
    lens = [[2, (4, 6), 5, (1, 3)], [(4, 4), 3, None, (1, 2)], (2, 5)]
    ends = [[None, a, None, b_], [b_], a]
    tabs = check_lines(lens, ends, 3, length, SENT, 160, prefix=pre)
    with pytest.raises(ValueError, match="more than its hi"):
        GreedyDecoder(model, 3, max_len=length).begin(tb, length, prefix=pre, line_lengths=[[2, 2], None, None])
    for n in (0, 3):
        ids = GreedyDecoder(model, 3, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, prefix=pre,
                                                               line_lengths=lens, line_end_ids=ends, no_repeat_ngram_size=n).cpu()
        for b, p in enumerate(pre):
            assert ids[b, :len(p)].tolist() == p
        assert all_violations(ids, tabs, pre, n=n) == []
        got = [line_lengths_of(r) for r in ids.tolist()]
        given = sum(1 for v in line[1:-1] if v != 0)
        assert 4 <= got[0][1] <= 6 and got[1][0] == 4 and got[0][0] == given != 2  # the whole given line is the caller's text
        if mode == "f32":
            for b in range(3):
                assert ids[b].tolist() == cpu_lines_greedy(w, sh, table, start_row(batch, b), length, tabs, b=b, n=n, prefix=pre[b]), (n, b)
        bids, _ = BeamDecoder(model, 3, 4, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, prefix=pre,
                                                                    line_lengths=lens, line_end_ids=ends, no_repeat_ngram_size=n)
        flat = bids.reshape(12, -1).cpu()
        for r in range(12):
            assert flat[r, :len(pre[r // 4])].tolist() == pre[r // 4]
            assert rule_violations(flat[r].tolist(), tabs, r // 4, start=len(pre[r // 4]), n=n) == []


# ------------------------------------------------------------------ 4. off means off
def test_none_is_exactly_the_call_without_the_arguments_and_unconstrained_tables_give_the_same_ids():
    model, tb = build("tiny_s5", "bf16")
    fresh = GreedyDecoder(model, 3)
    dec = GreedyDecoder(model, 3)
    a = fresh.generate(tb, 220, temperature=T, repitition_penalty=REP)
    b = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, line_lengths=None, line_end_ids=None)
    assert torch.equal(a, b) and set(dec.graphs) == set(fresh.graphs) and all("lines" not in k for k in dec.graphs)
    assert dec.kernel_name() == fresh.kernel_name() and dec.describe() == fresh.describe() and dec.rules.lines is None
    c = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, line_lengths=[None])           # the *_lines entries, no bounds
    assert torch.equal(a, c) and any("lines" in k for k in dec.graphs)
    kw = dict(temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7)
    sa = fresh.generate(tb, 220, generator=torch.Generator(device=DEV).manual_seed(5), **kw)
    sb = dec.generate(tb, 220, generator=torch.Generator(device=DEV).manual_seed(5), line_lengths=(0, CAP), **kw)
    sc = dec.generate(tb, 220, generator=torch.Generator(device=DEV).manual_seed(5), no_repeat_ngram_size=3, **kw)
    sd = dec.generate(tb, 220, generator=torch.Generator(device=DEV).manual_seed(5), no_repeat_ngram_size=3, line_lengths=[None], **kw)
    assert torch.equal(sa, sb) and torch.equal(sc, sd)
    bd, fb = BeamDecoder(model, 3, 4), BeamDecoder(model, 3, 4)
    ia, sa = fb.generate(tb, 220, temperature=T, repitition_penalty=REP)
    ib, sb = bd.generate(tb, 220, temperature=T, repitition_penalty=REP, line_lengths=None)
    assert torch.equal(ia, ib) and torch.equal(sa, sb) and set(bd.graphs) == set(fb.graphs) and bd.describe() == fb.describe()
    ic, sc = bd.generate(tb, 220, temperature=T, repitition_penalty=REP, line_lengths=(0, CAP))
    assert torch.equal(ia, ic) and torch.equal(sa, sc)
    # after a constrained run, None is the plain decoder again
    dec.generate(tb, 220, temperature=T, repitition_penalty=REP, line_lengths=7)
    assert torch.equal(dec.generate(tb, 220, temperature=T, repitition_penalty=REP), a) and dec.rules.lines is None


# ------------------------------------------------------------------ 5. full size
def test_full_size_bf16_under_the_rule_is_bit_stable():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    B, Ln, n = 256, 220, 3
    nbt = synth.make_batch(B, mcfg, dcfg, V, seed=13)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    rng = np.random.RandomState(4)
    sets = [frozenset(int(v) for v in rng.choice(np.arange(200, V), size=k, replace=False)) for k in (1, 40, 700, 3000)]
    lens, ends = [], []
    for b in range(B):
        lo = rng.randint(0, 8, size=10)
        hi = np.minimum(CAP, lo + rng.randint(0, 9, size=10))
        lens.append([(int(a), int(z)) for a, z in zip(lo, hi)])
        ends.append([sets[rng.randint(4)] if (l % 2 == 1 and hi[l] > 0) else None for l in range(10)])
    lens[5], ends[5] = None, None                                              # an unconstrained row among them
    tabs = check_lines(lens, ends, B, Ln, SENT, V)
    dec = GreedyDecoder(model, B, max_len=Ln, lanes=1)
    assert dec.fused and dec.use_graph
    two = GreedyDecoder(model, B, max_len=Ln, lanes=2)
    plain = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP)
    assert len(all_violations(plain, tabs)) > B // 2                           # the unconstrained run breaks what it then gets
    for kw in (dict(), dict(top_k=10, top_p=0.7)):
        gen = lambda: torch.Generator(device=DEV).manual_seed(21) if kw else None     # noqa: E731
        args = dict(temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n, line_lengths=tabs, **kw)
        g1 = dec.generate(batch, Ln, generator=gen(), **args)
        assert torch.equal(dec.generate(batch, Ln, generator=gen(), **args), g1), kw
        ge = dec.generate(batch, Ln, generator=gen(), use_graph=False, **args)
        assert torch.equal(ge, g1), kw
        g2 = two.generate(batch, Ln, generator=gen(), **args)
        assert torch.equal(g2, g1), kw
        assert all_violations(g1, tabs, n=n) == [], kw
        assert int(g1.min()) >= 0 and int(g1.max()) < V
        if not kw:
            assert torch.equal(g1[5], dec.generate(batch, Ln, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n)[5])
    bd = BeamDecoder(model, 64, 4, max_len=Ln)
    pb = {k: v[:64] for k, v in batch.items()}
    bt = check_lines(lens[:64], ends[:64], 64, Ln, SENT, V)
    i1, s1 = bd.generate(pb, Ln, temperature=T, repitition_penalty=REP, line_lengths=bt)
    i2, s2 = bd.generate(pb, Ln, temperature=T, repitition_penalty=REP, line_lengths=bt, use_graph=False)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    flat = i1.reshape(256, -1).cpu().tolist()
    assert [r for r in range(256) if rule_violations(flat[r], bt, r // 4)] == []


# ------------------------------------------------------------------ 6. text surface
def test_generate_samples_and_beams_write_lines_of_the_requested_lengths():
    from mmtg_amd.generate import generate_beams, generate_samples
    fx = setup_case("tiny_s5")[0]
    model, tb = build("tiny_s5", "f32")
    names = {0: "[PAD]", 1: "[#START#]", 2: "[#EOS#]", 100: "[UNK]", 102: "[SEP]"}

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [names.get(int(i), chr(0x4e00 + int(i))) for i in ids]

    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    plain = generate_samples(model, rows, Tok(), n_samples=1, length=220, top_k=1, top_p=0.0)
    assert all(len(p) != 7 for t in plain for p in t[0].split("，"))           # the fixture writes 20-token or empty lines ...
    texts = generate_samples(model, rows, Tok(), n_samples=4, length=220, line_lengths=7)
    assert len(texts) == 3 and all(len(t) == 4 for t in texts)
    for t in texts:
        for s in t:
            assert [len(p) for p in s.split("，")] == [7] * 10, s                # ... and seven-token lines on request
    a, _ = end_sets_for(fx)
    chars = {chr(0x4e00 + v) for v in a}
    form = [[5, 7, 5, 7, 5, 7], [(1, 4)] * 6, None]                             # per prompt
    out = generate_beams(model, rows, Tok(), num_beams=4, length=6 * SENT, line_lengths=form, line_end_ids=[None, a, None, a],
                         return_all=True)
    assert len(out) == 3 and all(len(b) == 4 for b in out)
    for text, score in out[0]:
        parts = text.split("，")
        assert [len(p) for p in parts] == [5, 7, 5, 7, 5, 7] and parts[1][-1] in chars and parts[3][-1] in chars and np.isfinite(score)
    for text, _ in out[1]:
        parts = text.split("，")
        assert len(parts) == 6 and all(1 <= len(p) <= 4 for p in parts) and parts[1][-1] in chars and parts[3][-1] in chars
