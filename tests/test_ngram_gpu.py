"""n-gram blocking on the MI355X: the *_ngram selection entries against their plain / *_fixed namesakes on pre-banned logits, the
decoders (GreedyDecoder / BeamDecoder with no_repeat_ngram_size=n) against the CPU restatements of tests/test_ngram_cpu.py, prefixes,
n = 0, full-size determinism and the text surface (generate_samples / generate_beams)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import batch_to_torch, load_case  # noqa: E402
from mmtg_amd import MMTG, hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case, start_row  # noqa: E402
from test_ngram_cpu import banned_ids, cpu_ngram_beam_search, cpu_ngram_greedy, repeated_ngrams, violations  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402

DEV = "cuda"


def build(case, mode):
    fx, meta, mcfg, gcfg, dcfg, weights, table, batch = load_case(case)
    model = MMTG(mcfg, dcfg, meta["V"], train_flag=False, gpt2_config=gcfg, token_table=table, compute_dtype=mode)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    model.to(DEV).eval()
    tb = {k: v for k, v in batch_to_torch(batch, DEV).items() if k not in ("rating", "targets")}
    return model, tb


def full_size_model(mode="bf16"):
    from mmtg_amd import synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype=mode,
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to(DEV).eval()
    return model, mcfg, dcfg, V


def free_violations(ids, n, prefixes=None):
    """Rows of ids [B, 1 + length] with a column (after the row's prefix) that completes a content n-gram held earlier."""
    ids = ids.cpu().tolist()
    return [b for b, r in enumerate(ids) if violations(r, n, start=len(prefixes[b]) if prefixes else 1)]


# ------------------------------------------------------------------ 1. kernels
def _histories(B, P, Tmax, g):
    """seq rows over a 4-id alphabet (content ids 3..5 and PAD) so that n-grams repeat, some rows with [#EOS#] / [#START#] inside."""
    seq = torch.randint(3, 6, (B, Tmax), generator=g)
    seq[torch.rand(B, Tmax, generator=g) < 0.08] = 0
    seq[:, P] = 1
    seq[1, P + 6:P + 9] = torch.tensor([2, 1, 100])
    seq[2, P + 1:P + 7] = torch.tensor([3, 4, 5, 3, 4, 5])                    # a copied phrase
    return seq


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ngram_entries_equal_their_namesakes_on_pre_banned_logits(n):
    """Each *_ngram entry writes bit for bit what its plain (fixed_end None) or *_fixed namesake writes on the same logits with the
    row's banned ids (test_ngram_cpu.banned_ids of its history) set to -inf beforehand: ids for greedy, ids for sampling with the same
    uniforms, candidate values and ids for beams.  Covers sticky-PAD rows, forced columns and held prefix rows."""
    B, P, V, Vp, Tmax, nb = 8, 5, 160, 168, 64, 4
    g = torch.Generator().manual_seed(100 + n)
    logits = torch.randn(B, Vp, generator=g) * 2
    logits[:, 3:6] += 6.0                                                     # the repeating ids are the likely ones
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24).to(DEV)
    seq0 = _histories(B, P, Tmax, g)
    hits = 0
    for pos in (P + 10, P + 15, P + 20, P + 21, P + 30):                      # model calls, [#EOS#], [#START#]
        j = pos + 1 - P
        s0 = seq0.clone()
        s0[5, P + j - 1] = 0                                                  # a sticky-PAD row
        masked = logits.clone()
        for b in range(B):
            ban = sorted(banned_ids(s0[b, P:P + j].tolist(), n))
            hits += len(ban)
            masked[b, ban] = float("-inf")
        s0, lg, mk = s0.to(DEV), logits.to(DEV), masked.to(DEV)
        for fe in (None, torch.tensor([0, pos + 2, 0, pos + 1, 0, 0, pos + 5, 0], dtype=torch.int32, device=DEV)):
            for kind in ("select", "sample"):
                a, b_ = s0.clone(), s0.clone()
                pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
                if kind == "select":
                    if fe is None:
                        hip.decode_select(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, B, pos_next=pa[1:2])
                    else:
                        hip.decode_select_fixed(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, B, fe, pos_next=pa[1:2])
                    hip.decode_select_ngram(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, B, n, fixed_end=fe, pos_next=pb[1:2])
                else:
                    if fe is None:
                        hip.decode_sample(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, pos_next=pa[1:2])
                    else:
                        hip.decode_sample_fixed(mk, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, fe, pos_next=pa[1:2])
                    hip.decode_sample_ngram(lg, Vp, V, b_, pb[0:1], P, SENT, T, REP, 10, 0.7, uni, B, n, fixed_end=fe, pos_next=pb[1:2])
                torch.cuda.synchronize()
                assert int(pb[1]) == pos + 1 == int(pa[1])
                assert torch.equal(a, b_), (pos, kind, fe is None)
            cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
            cvb, cib = cva.clone(), cia.clone()
            pp = torch.tensor([pos], dtype=torch.int32, device=DEV)
            if fe is None:
                hip.decode_beam_candidates(mk, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B)
            else:
                hip.decode_beam_candidates_fixed(mk, Vp, V, s0, pp, P, SENT, T, REP, nb, cva, cia, B, fe)
            hip.decode_beam_candidates_ngram(lg, Vp, V, s0, pp, P, SENT, T, REP, nb, cvb, cib, B, n, fixed_end=fe)
            torch.cuda.synchronize()
            assert torch.equal(cva, cvb) and torch.equal(cia, cib), (pos, fe is None)
    assert hits > 0


# ------------------------------------------------------------------ 2. model level
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_greedy_with_bans_is_the_cpu_restatement(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    dec = GreedyDecoder(model, 3, max_len=220)
    for n, length in ((2, 140), (3, 220)):
        ids = dec.generate(tb, length, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n).cpu()
        assert not free_violations(ids, n)
        for row in range(3):
            want = cpu_ngram_greedy(w, sh, table, start_row(batch, row), length, n)
            assert ids[row].tolist() == want, (n, row)
    assert ("ngram", 3) in {k[-2:] for k in dec.graphs}


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_four_beams_with_bans_follow_the_cpu_beam_search(mode):
    nb, full, n = 4, 110, 2
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    lens = []
    for row in range(3):
        _, _, gaps = cpu_ngram_beam_search(w, sh, table, start_row(batch, row), full, nb, n)
        lens.append(comparable_length(gaps, full))
    assert max(lens) >= 40, lens
    dec = BeamDecoder(model, 3, nb, max_len=full)
    runs = {}
    for row, L in enumerate(lens):
        if L < 1:
            continue
        if L not in runs:
            runs[L] = [t.cpu() for t in dec.generate(tb, L, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n)]
        ids, scores = runs[L]
        cids, cscores, _ = cpu_ngram_beam_search(w, sh, table, start_row(batch, row), L, nb, n)
        assert ids[row].tolist() == cids.tolist(), (row, L)
        np.testing.assert_allclose(scores[row].numpy(), cscores, rtol=0, atol=1e-3)
        assert not free_violations(ids[row], n)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_one_beam_with_bans_is_greedy_with_bans(mode):
    model, tb = build("tiny_s5", mode)
    for n in (1, 2, 4):
        greedy = GreedyDecoder(model, 3).generate(tb, 220, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n)
        ids, scores = BeamDecoder(model, 3, 1).generate(tb, 220, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=n)
        assert torch.equal(ids[:, 0], greedy), n
        assert torch.isfinite(scores).all() and not free_violations(greedy, n)


# ------------------------------------------------------------------ 3. with a prefix
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_bans_with_a_prefix_count_the_prefix(mode):
    """Prefix columns come back unchanged (a prefix may repeat itself); the free columns obey the rule with the prefix in the
    history; in f32 the ids are the CPU restatement started from the prefix; beams too."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    line = batch["targets"][0, :SENT].tolist()
    pre = [batch["targets"][0, :SENT + 1].tolist(), line + [1] + line[1:6], [1]]   # row 1 copies the start of its first line
    length = 100
    for n in (2, 3):
        ids = GreedyDecoder(model, 3, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, prefix=pre,
                                                               no_repeat_ngram_size=n).cpu()
        for b, p in enumerate(pre):
            assert ids[b, :len(p)].tolist() == p
        assert not free_violations(ids, n, pre), n
        if mode == "f32":
            for b in range(3):
                assert ids[b].tolist() == cpu_ngram_greedy(w, sh, table, start_row(batch, b), length, n, prefix=pre[b]), (n, b)
        bids, _ = BeamDecoder(model, 3, 4, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, prefix=pre,
                                                                    no_repeat_ngram_size=n)
        flat = bids.reshape(12, -1)
        rpre = [p for p in pre for _ in range(4)]
        for r in range(12):
            assert flat[r, :len(rpre[r])].tolist() == rpre[r]
        assert not free_violations(flat, n, rpre), n


# ------------------------------------------------------------------ 4. off means off
def test_zero_is_exactly_the_call_without_the_argument():
    model, tb = build("tiny_s5", "bf16")
    dec = GreedyDecoder(model, 3)
    a = dec.generate(tb, 220, temperature=T, repitition_penalty=REP)
    b = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=0)
    assert torch.equal(a, b)
    kw = dict(temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7)
    a = dec.generate(tb, 220, generator=torch.Generator(device=DEV).manual_seed(5), **kw)
    b = dec.generate(tb, 220, generator=torch.Generator(device=DEV).manual_seed(5), no_repeat_ngram_size=0, **kw)
    assert torch.equal(a, b)
    assert all("ngram" not in k for k in dec.graphs)
    bd = BeamDecoder(model, 3, 4)
    ia, sa = bd.generate(tb, 220, temperature=T, repitition_penalty=REP)
    ib, sb = bd.generate(tb, 220, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=0)
    assert torch.equal(ia, ib) and torch.equal(sa, sb)
    # after a run with bans, n = 0 is the plain decoder again
    dec.generate(tb, 220, temperature=T, repitition_penalty=REP, no_repeat_ngram_size=1)
    assert torch.equal(dec.generate(tb, 220, temperature=T, repitition_penalty=REP),
                       GreedyDecoder(model, 3).generate(tb, 220, temperature=T, repitition_penalty=REP))


# ------------------------------------------------------------------ 5. full size
def test_full_size_bf16_with_four_gram_bans_is_bit_stable():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    B, Ln, n = 256, 220, 4
    nbt = synth.make_batch(B, mcfg, dcfg, V, seed=13)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    dec = GreedyDecoder(model, B, max_len=Ln, lanes=1)
    assert dec.fused and dec.use_graph
    two = GreedyDecoder(model, B, max_len=Ln, lanes=2)
    kws = (dict(), dict(top_k=10, top_p=0.7))
    for kw in kws:
        gen = lambda: torch.Generator(device=DEV).manual_seed(21) if kw else None     # noqa: E731
        g1 = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP, generator=gen(), no_repeat_ngram_size=n, **kw)
        ge = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP, generator=gen(), no_repeat_ngram_size=n, use_graph=False, **kw)
        assert torch.equal(ge, g1), kw
        g2 = two.generate(batch, Ln, temperature=T, repitition_penalty=REP, generator=gen(), no_repeat_ngram_size=n, **kw)
        assert torch.equal(g2, g1), kw
        assert not free_violations(g1, n), kw
        assert not any(repeated_ngrams(r, n) for r in g1.cpu().tolist())
        assert int(g1.min()) >= 0 and int(g1.max()) < V


# ------------------------------------------------------------------ 6. text surface
def test_generate_samples_and_beams_obey_the_rule():
    from mmtg_amd.generate import generate_beams, generate_samples
    model, tb = build("tiny_s5", "f32")
    seen = []

    class Tok:
        def convert_ids_to_tokens(self, ids):
            seen.append([int(i) for i in ids])
            return ["tok%d" % int(i) for i in ids]

    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    texts = generate_samples(model, rows, Tok(), n_samples=4, length=220, no_repeat_ngram_size=3)
    assert len(texts) == 3 and all(len(t) == 4 for t in texts) and len(seen) == 12
    assert not any(violations(r, 3) for r in seen)
    seen.clear()
    out = generate_beams(model, rows, Tok(), num_beams=4, length=220, no_repeat_ngram_size=3, return_all=True)
    assert len(out) == 3 and len(seen) == 12
    assert not any(violations(r, 3) for r in seen)
    seen.clear()
    plain = generate_samples(model, rows, Tok(), n_samples=1, length=220, top_k=1, top_p=0.0)
    assert repeated_ngrams(seen[1], 2)                                        # the fixture repeats bigrams ...
    seen.clear()
    banned = generate_samples(model, rows, Tok(), n_samples=1, length=220, top_k=1, top_p=0.0, no_repeat_ngram_size=2)
    assert not any(repeated_ngrams(r, 2) for r in seen) and banned != plain  # ... which n = 2 removes
