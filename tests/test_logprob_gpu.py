"""Token log-probabilities on the MI355X: mmtg_decode_logprob against torch in float64, the decoders with return_logprobs= against
the logits each step saw, rule-independence under every constraint at once, the scoring mode (generate.score_sequences), beams, the
text surface (generate_samples with return_scores= / rank_by=) and the full vocabulary once."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import batch_to_torch, load_case  # noqa: E402
from mmtg_amd import MMTG, hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder, chosen_mask, sequence_scores  # noqa: E402
from mmtg_amd.generate import generate_samples, score_sequences  # noqa: E402

DEV = "cuda"
SENT = 22
T, REP = 1.1, 1.5
ATOL = 1e-4     # per-thread sums of <= 52 terms + a tree: ~4e-6 relative; |x - max| <= ~50 rounded at 2^-24: ~3e-6; expf / logf a few
                # ulp; together ~2e-5, with a 5x margin
PARITY = {"f32": 2e-3, "bf16x3": 2e-3, "bf16": 0.3}     # twice the mode's logits parity bound (README): a logit minus an LSE


def build(case, mode):
    fx, meta, mcfg, gcfg, dcfg, weights, table, batch = load_case(case)
    model = MMTG(mcfg, dcfg, meta["V"], train_flag=False, gpt2_config=gcfg, token_table=table, compute_dtype=mode)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    model.to(DEV).eval()
    tb = {k: v for k, v in batch_to_torch(batch, DEV).items() if k not in ("rating", "targets")}
    return model, tb


def reference(logits, V, ids):
    """log_softmax(logits[:, :V]) in float64 gathered at ids [B]."""
    return torch.log_softmax(logits[:, :V].double(), dim=1).gather(1, ids.view(-1, 1).long()).view(-1)


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("V,ldl", [(5, 8), (160, 168), (161, 161), (13317, 13320), (16387, 16392)])
def test_kernel_is_the_float64_log_softmax_at_the_placed_id(V, ldl):
    """(5, 8): the tail loop only; (160, 168): the other selection tests' shape; (161, 161): rows 1, 2, 3, 5, ... unaligned, the scalar
    path; (13317, 13320): the real cut, 3329 vectors + a tail of 1 in one load pass; (16387, 16392): a second load pass."""
    B, P, ld, ncols = 8, 5, 64, 45
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(B, ldl, generator=g) * 4
    logits[torch.rand(B, ldl, generator=g) < 0.1] = float("-inf")
    ids = torch.randint(0, V, (B,), generator=g)
    for b in range(B):
        if b not in (2, 3):
            logits[b, ids[b]] = float(b) - 3.0                                # a finite chosen entry ...
    logits[2, ids[2]] = float("-inf")                                         # ... but row 2's, which is -inf
    logits[3] = float("-inf")                                                 # a row without a distribution
    if V > 5:
        logits[4, :V] = float("-inf")
        logits[4, ids[4]] = 1.5                                               # one live entry: log-probability 0
    pos = P + 9
    j = pos + 1 - P
    seq = torch.randint(0, V, (B, ld), generator=g)
    seq[:, pos + 1] = ids
    seq[6, pos + 1] = V                                                       # an id outside the cut: nothing is written
    want = reference(logits, V, ids)
    logits, seq = logits.to(DEV), seq.to(DEV)
    pp = torch.tensor([pos, P + ncols - 1, -1], dtype=torch.int32, device=DEV)
    out = torch.full((B, ncols), 7.0, device=DEV)
    hip.decode_logprob(logits, ldl, V, seq, pp[0:1], P, out, B)
    again = torch.full((B, ncols), 7.0, device=DEV)
    hip.decode_logprob(logits, ldl, V, seq, pp[0:1], P, again, B)
    edge = torch.full((B, ncols), 7.0, device=DEV)
    hip.decode_logprob(logits, ldl, V, seq, pp[1:2], P, edge, B)              # j == ncols: past the table
    hip.decode_logprob(logits, ldl, V, seq, pp[2:3], P, edge, B)              # j < 0
    torch.cuda.synchronize()
    out, again, edge = out.cpu(), again.cpu(), edge.cpu()
    assert int(pp[0]) == pos
    assert torch.equal(edge, torch.full((B, ncols), 7.0))
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))        # bit-equal
    rest = torch.ones(ncols, dtype=torch.bool)
    rest[j] = False
    assert torch.equal(out[:, rest], torch.full((B, ncols - 1), 7.0))         # only column pos + 1 - P changes
    assert out[6, j] == 7.0
    got = out[:, j]
    assert not torch.isnan(got).any()
    assert got[2] == float("-inf") and got[3] == float("-inf")
    if V > 5:
        assert got[4] == 0.0
    live = [b for b in range(B) if b not in (2, 3, 6)]
    err = (got[live].double() - want[live]).abs().max().item()
    print("V %d ldl %d: max |error| %.3g" % (V, ldl, err))
    assert torch.isfinite(got[live]).all() and err <= ATOL


# ------------------------------------------------------------------ 2. the decoders
def tapped(dec, tb, length, **kw):
    """(ids, tok_lp, {j: the logits the step saw}) of one generation with return_logprobs."""
    seen = {}

    def tap(j, with_head, picked, logits):
        if with_head:
            seen[j] = logits.clone()
        else:
            assert logits is None
    ids, lp = dec.generate(tb, length, tap=tap, return_logprobs=True, **kw)
    return ids, lp, seen


def check_against_taps(ids, lp, seen, V, length, first_col=1):
    """tok_lp[:, j] is the float64 log-softmax of the step's logits at the id the column holds, on every head step; exactly 0 on
    column 0, the cadence columns and every other column no head step wrote.  Returns the largest error."""
    head = sorted(seen)
    assert head == [j for j in range(first_col, length + 1) if j % SENT not in (0, SENT - 1)]
    worst = 0.0
    for j in head:
        want = reference(seen[j], V, ids[:, j])
        worst = max(worst, (lp[:, j].double() - want).abs().max().item())
    quiet = [j for j in range(length + 1) if j not in seen]
    assert 0 in quiet and SENT - 1 in quiet and SENT in quiet
    assert (lp[:, quiet] == 0).all()
    assert lp.shape == (ids.shape[0], length + 1) and lp.dtype == torch.float32
    return worst


@pytest.mark.parametrize("sampling", [False, True])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "f32"])
@pytest.mark.parametrize("case", ["tiny_s2", "tiny_lstm2_rnn2"])
def test_decoder_logprobs_are_the_tapped_logits_and_leave_the_ids_alone(case, mode, sampling):
    model, tb = build(case, mode)
    B, length = tb["img_embs"].shape[0], 2 * SENT + 3
    dec = GreedyDecoder(model, B, max_len=length, lanes=1)
    kw = dict(temperature=T, repitition_penalty=REP, **(dict(top_k=10, top_p=0.7) if sampling else {}))
    gen = lambda: torch.Generator(device=DEV).manual_seed(11) if sampling else None     # noqa: E731
    for use_graph in (True, False):
        plain = dec.generate(tb, length, generator=gen(), use_graph=use_graph, **kw)
        keys = set(dec.graphs)
        assert not use_graph or all("logprob" not in k for k in keys)
        ids, lp, seen = tapped(dec, tb, length, generator=gen(), use_graph=use_graph, **kw)
        assert torch.equal(ids, plain)                                        # bit-equal to the call without the argument
        err = check_against_taps(ids, lp, seen, 160, length)
        print("%s %s sampling %s graph %s: max |error| %.3g" % (case, mode, sampling, use_graph, err))
        assert err <= ATOL
        assert (lp[:, sorted(seen)] < 0).all()
        if use_graph:                                                         # the head steps got graphs of their own, the others not
            new = set(dec.graphs) - keys
            assert new and all(k[0] and k[-1] == "logprob" for k in new)
    assert torch.equal(dec.generate(tb, length, generator=gen(), **kw), plain)     # and off is the plain decoder again


# ------------------------------------------------------------------ 3. whatever decided the column
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_logprobs_score_whatever_the_column_holds(mode):
    """Prefixes of different lengths, 2-gram bans, a template with a given column, bounds that fill lines and a rhyme scheme in one
    generation: every column a head step wrote holds the model's log-probability of the id it holds -- a pick, a given id, a
    full line's PAD, a sticky PAD, a held prefix id."""
    model, tb = build("tiny_s5", mode)
    length = 2 * SENT
    pre = [[1, 20], [1, 20, 31, 32], [1, 20, 33]]
    kw = dict(temperature=T, repitition_penalty=REP, prefix=pre, no_repeat_ngram_size=2, line_lengths=(1, 5),
              templates=[None, (25, None, Ellipsis)], rhyme_scheme="AA", rhyme_classes=[set(range(10, 20)), set(range(30, 40))])
    dec = GreedyDecoder(model, 3, max_len=length, lanes=1)
    plain = dec.generate(tb, length, **kw)
    for extra in (dict(), dict(top_k=10, top_p=0.7, generator=torch.Generator(device=DEV).manual_seed(3))):
        ids, lp, seen = tapped(dec, tb, length, **kw, **extra)
        if not extra:
            assert torch.equal(ids, plain)
        err = check_against_taps(ids, lp, seen, 160, length, first_col=2)     # the prefill covers column 1 of every row
        print("%s %s: max |error| %.3g" % (mode, "sampled" if extra else "greedy", err))
        assert err <= ATOL
        rows = ids.cpu().tolist()
        for b, p in enumerate(pre):
            assert rows[b][:len(p)] == p
        assert (lp[:, 1] == 0).all()
        assert (lp[1, 2:4] < 0).all() and lp[2, 2] < 0                        # held prefix columns of the longer prefixes
        assert all(r[SENT + 1] == 25 for r in rows) and (lp[:, SENT + 1] < 0).all()     # the template's given column
        assert all(r[6] == 0 for r in rows) and (lp[:, 6] < 0).all()          # hi = 5: the line is full, PAD
        assert (lp[:, 7:SENT - 1] < 0).all()                                  # sticky PADs: the model's log-probability of PAD


# ------------------------------------------------------------------ 4. scoring given text
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_score_sequences_returns_what_the_generation_reported(mode):
    model, tb = build("tiny_s2", mode)
    B, length = tb["img_embs"].shape[0], 2 * SENT + 3
    dec = GreedyDecoder(model, B, max_len=length, lanes=1)
    ids, lp = dec.generate(tb, length, temperature=T, repitition_penalty=REP, return_logprobs=True)
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    got = score_sequences(model, rows, ids)
    assert got.shape == (B, length + 1) and got.dtype == np.float32
    back, again = dec.generate(tb, length, prefix=ids.cpu().tolist(), return_logprobs=True)     # the mode score_sequences runs
    assert torch.equal(back, ids)                                             # the ids come back unchanged
    head = [j for j in range(1, length + 1) if j % SENT not in (0, SENT - 1)]
    quiet = [j for j in range(length + 1) if j not in head]
    diff = np.abs(got[:, head].astype(np.float64) - lp[:, head].cpu().numpy()).max()
    print("%s: scoring mode against the generation, max |difference| %.3g (bound %.3g)" % (mode, diff, PARITY[mode]))
    assert diff <= PARITY[mode]
    assert (got[:, quiet] == 0).all() and (got[:, head] < 0).all()
    assert np.array_equal(got, again.cpu().numpy())
    small = score_sequences(model, rows, ids, max_batch=3)                    # chunked, the last chunk padded
    assert np.abs(small.astype(np.float64) - got).max() <= PARITY[mode]
    # a prefix every row shares goes through the prefill: the generation leaves its columns 0, the scoring mode does not
    _, part = dec.generate(tb, length, temperature=T, repitition_penalty=REP, prefix=ids[:, :4].cpu().tolist(), return_logprobs=True)
    assert (part[:, :4] == 0).all() and (part[:, 4] < 0).all()
    assert (got[:, 1:4] < 0).all()


# ------------------------------------------------------------------ 5. beams
def test_beam_decoder_refuses_logprobs_before_any_device_work():
    model, tb = build("tiny_s5", "bf16")
    bd = BeamDecoder(model, 3, 2, max_len=SENT)
    with pytest.raises(ValueError, match="return_logprobs"):
        bd.generate(None, SENT, return_logprobs=True)                         # the batch is never looked at
    with pytest.raises(ValueError, match="return_logprobs"):
        bd.begin(None, SENT, return_logprobs=True)
    ids, scores = bd.generate(tb, SENT, temperature=T, repitition_penalty=REP)
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    lp = score_sequences(model, rows, ids[:, 0])                              # a beam is scored afterwards
    s, c = sequence_scores(ids[:, 0], lp, sent=SENT)
    assert np.isfinite(s).all() and (s < 0).all() and (c > 0).all()

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return ["tok%d" % int(i) for i in ids]

    from mmtg_amd.generate import generate_beams
    kw = dict(num_beams=2, length=SENT, temperature=T, repetition_penalty=REP, return_all=True)
    beams = generate_beams(model, rows, Tok(), return_ids=True, **kw)         # the text surface hands the ids on
    assert [[b[:2] for b in e] for e in beams] == generate_beams(model, rows, Tok(), **kw)
    assert [e[0][2] for e in beams] == ids[:, 0].cpu().tolist()
    assert np.array_equal(score_sequences(model, rows, [e[0][2] for e in beams]), lp)


# ------------------------------------------------------------------ 6. the text surface
def test_generate_samples_scores_and_ranks_without_changing_the_texts():
    model, tb = build("tiny_s5", "f32")
    length, n = 2 * SENT + 3, 4

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return ["tok%d" % int(i) for i in ids]

    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)      # noqa: E731
    plain = generate_samples(model, rows, Tok(), n_samples=n, length=length, generator=gen())
    scored = generate_samples(model, rows, Tok(), n_samples=n, length=length, generator=gen(), return_scores=True)
    assert [[t for t, _, _ in e] for e in scored] == plain                    # the same strings from the same seed
    rep = {k: v.repeat_interleave(n, dim=0) for k, v in tb.items()}
    ids, lp = GreedyDecoder(model, 3 * n, max_len=length).generate(rep, length, temperature=1.1, repitition_penalty=1.5, top_k=10,
                                                                 top_p=0.7, generator=gen(), return_logprobs=True)
    upto = len(GreedyDecoder.reference_return(ids[0].tolist(), length, sent=SENT))
    assert upto == length                                                     # the last iteration's append is not part of the text
    sums, counts = sequence_scores(ids, lp, sent=SENT, upto=upto)
    mask = chosen_mask(ids, sent=SENT)
    mask[:, upto:] = False
    flat = [t for e in scored for t in e]
    assert [c for _, _, c in flat] == mask.sum(1).tolist() == counts.tolist()
    assert [s for _, s, _ in flat] == [float(v) for v in sums]
    assert all(s < 0 and c > 0 for _, s, c in flat)
    for by, key in (("mean", lambda t: t[1] / max(t[2], 1)), ("sum", lambda t: t[1])):
        ranked = generate_samples(model, rows, Tok(), n_samples=n, length=length, generator=gen(), rank_by=by)
        for e, r in zip(scored, ranked):
            assert sorted(e) == sorted(r)
            ks = [key(t) for t in r]
            assert all(a >= b for a, b in zip(ks, ks[1:]))                    # best first
    with pytest.raises(ValueError, match="rank_by"):
        generate_samples(model, rows, Tok(), n_samples=n, length=length, rank_by="best")
    # a prompt's prefix is not scored
    pre = [[1, 20, 21], [1, 22], [1]]
    out = generate_samples(model, rows, Tok(), n_samples=2, length=length, generator=gen(), prefixes=pre, return_scores=True)
    ids, lp = GreedyDecoder(model, 6, max_len=length).generate({k: v.repeat_interleave(2, dim=0) for k, v in tb.items()}, length,
                                                               temperature=1.1, repitition_penalty=1.5, top_k=10, top_p=0.7,
                                                               generator=gen(), prefix=[p for p in pre for _ in range(2)],
                                                               return_logprobs=True)
    sums, counts = sequence_scores(ids, lp, sent=SENT, prefix_lens=[3, 3, 2, 2, 1, 1], upto=length)
    assert [(s, c) for e in out for _, s, c in e] == [(float(s), int(c)) for s, c in zip(sums, counts)]


# ------------------------------------------------------------------ 7. the full vocabulary
def test_full_vocabulary_bf16_graph_replay_is_the_tapped_logits_and_bit_stable():
    from mmtg_amd import synth
    from test_ngram_gpu import full_size_model
    model, mcfg, dcfg, V = full_size_model("bf16")
    B, length = 8, 2 * SENT
    nbt = synth.make_batch(B, mcfg, dcfg, V, seed=13)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    dec = GreedyDecoder(model, B, max_len=length, lanes=1)
    assert dec.use_graph and V == 13317
    ids, lp, seen = tapped(dec, batch, length, temperature=T, repitition_penalty=REP)
    err = check_against_taps(ids, lp, seen, V, length)
    print("full vocabulary: max |error| %.3g" % err)
    assert err <= ATOL
    ids2, lp2 = dec.generate(batch, length, temperature=T, repitition_penalty=REP, return_logprobs=True)
    assert torch.equal(ids2, ids) and torch.equal(lp2.view(torch.int32), lp.view(torch.int32))
    assert any(k[-1] == "logprob" for k in dec.graphs)
