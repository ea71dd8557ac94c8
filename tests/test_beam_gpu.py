"""Beam search on the KV-cached, graph-replayed decoder (mmtg_amd.decode.BeamDecoder) on the MI355X: one beam is greedy, the beams
follow the CPU beam search of tests/test_beam_cpu.py, every returned score re-scores through the greedy decoder, the table-aware
attention and the selection kernels against torch restatements, and the full-size run's determinism."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import batch_to_torch, load_case  # noqa: E402
from mmtg_amd import MMTG, hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, comparable_length, cpu_beam_search, setup_case, start_row  # noqa: E402

DEV = "cuda"
T, REP = 1.1, 1.5


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


# ------------------------------------------------------------------ 3. one beam is greedy
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", ["tiny_s5", "full_12l"])
def test_one_beam_is_the_greedy_decoder(case, mode):
    model, tb = build(case, mode)
    n = tb["img_embs"].shape[0]
    length = 220
    greedy = GreedyDecoder(model, n).generate(tb, length, temperature=T, repitition_penalty=REP)
    dec = BeamDecoder(model, n, 1)
    assert dec.x3 == (mode == "bf16x3") and (mode != "bf16" or dec.fused)
    ids, scores = dec.generate(tb, length, temperature=T, repitition_penalty=REP)
    assert tuple(ids.shape) == (n, 1, 1 + length) and tuple(scores.shape) == (n, 1)
    assert torch.equal(ids[:, 0], greedy)
    assert torch.isfinite(scores).all() and (scores < 0).all()


# ------------------------------------------------------------------ 4. the beams are the CPU beam search's
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", ["tiny_s5", "tiny_lstm2_rnn2"])
def test_four_beams_follow_the_cpu_beam_search(case, mode):
    """Every prompt is compared over the generated positions before its first CPU selection whose nb-th / (nb+1)-th gap is below
    1e-4 (there two fp32 searches may order candidates differently): a run of that length, ids and beam order equal, scores
    within 1e-3."""
    nb, full = 4, 120
    fx, sh, w, table, batch = setup_case(case)
    model, tb = build(case, mode)
    n = tb["img_embs"].shape[0]
    lens = []
    for row in range(n):
        _, _, gaps = cpu_beam_search(w, sh, table, start_row(batch, row), full, nb, T, REP)
        lens.append(comparable_length(gaps, full))
    assert max(lens) >= 60, lens
    dec = BeamDecoder(model, n, nb, max_len=full)
    runs = {}
    for row, L in enumerate(lens):
        if L < 1:
            continue
        if L not in runs:
            runs[L] = [t.cpu() for t in dec.generate(tb, L, temperature=T, repitition_penalty=REP)]
        ids, scores = runs[L]
        cids, cscores, _ = cpu_beam_search(w, sh, table, start_row(batch, row), L, nb, T, REP)
        assert ids[row].tolist() == cids.tolist(), (row, L)
        np.testing.assert_allclose(scores[row].numpy(), cscores, rtol=0, atol=1e-3)


# ------------------------------------------------------------------ 5. every returned score re-scores through the greedy decoder
def rescore(model, tb, ids, length, V):
    """Teacher-force every beam through GreedyDecoder.generate and sum the fp32 log_softmax of the processed tapped logits at the
    positions the model chose (sticky PAD: 0)."""
    n, nb = ids.shape[:2]
    flat = ids.reshape(n * nb, -1).cpu()
    rep = {k: v.repeat_interleave(nb, 0) for k, v in tb.items()}
    g = GreedyDecoder(model, n * nb)
    acc = np.zeros(n * nb, np.float64)

    def tap(j, with_head, picked, logits):
        if not with_head:
            return
        lg = logits[:, :V].float().cpu()
        for r in range(n * nb):
            hist = flat[r, :j]
            if int(hist[-1]) == 0:
                assert int(flat[r, j]) == 0
                continue
            x = O.process_logits(lg[r], hist, T, REP)[:min(V, 13317)]
            acc[r] += float(torch.log_softmax(x, -1)[int(flat[r, j])])

    g.generate(rep, length, temperature=T, repitition_penalty=REP, teacher=flat, tap=tap)
    return acc.reshape(n, nb)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_returned_scores_rescore_through_the_greedy_decoder(mode):
    nb, length = 4, 120
    model, tb = build("tiny_s5", mode)
    n = tb["img_embs"].shape[0]
    ids, scores = BeamDecoder(model, n, nb, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP)
    sc = scores.cpu().numpy().astype(np.float64)
    assert np.isfinite(sc).all() and (np.diff(sc, axis=1) <= 0).all()
    got = rescore(model, tb, ids, length, model.engine().sh.V)
    np.testing.assert_allclose(got, sc, rtol=1e-3, atol=0)
    # every beam obeys the generation rules
    c = ids.cpu()
    for j in range(2, 1 + length):
        if (j + 1) % SENT == 0:
            assert (c[:, :, j] == 2).all()
        elif (j + 1) % SENT == 1:
            assert (c[:, :, j] == 1).all()
        else:
            assert not ((c[:, :, j] == 1) | (c[:, :, j] == 2) | (c[:, :, j] == 100) | (c[:, :, j] == 102)).any()
            assert (c[:, :, j][c[:, :, j - 1] == 0] == 0).all()


# ------------------------------------------------------------------ 6. kernels
def _attn_case(dtype, B=6, nH=12, Tmax=48, pos=37, splits=2, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = nH * 64
    part = torch.randn(splits, B, 3 * D, generator=g).to(DEV)
    bias = (0.1 * torch.randn(3 * D, generator=g)).to(DEV)
    kc = torch.randn(B, nH, Tmax, 64, generator=g).to(dtype).to(DEV)
    vc = torch.randn(B, nH, Tmax, 64, generator=g).to(dtype).to(DEV)
    keep = (torch.rand(B, Tmax, generator=g) > 0.2).to(torch.int32).to(DEV)
    rows = torch.randint(0, B, (B, Tmax), generator=g, dtype=torch.int32).to(DEV)
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    return part, bias, kc, vc, keep, rows, posd, B, nH, Tmax, pos, splits


def _run_attn(form, part, bias, kc, vc, keep, posd, B, nH, Tmax, splits, rows=None):
    kc, vc = kc.clone(), vc.clone()
    if form == "x3":
        out = hip.Planes.empty(B, nH * 64, DEV)
        hip.decode_attn_split_x3(part, splits, bias, kc, vc, keep, posd, out, B, nH, 64, Tmax, rows=rows)
        res = out.t.clone()
    else:
        out = torch.empty(B, nH * 64, dtype=kc.dtype, device=DEV)
        hip.decode_attn_split(part, splits, bias, kc, vc, keep, posd, out, B, nH, 64, Tmax, rows=rows)
        res = out
    torch.cuda.synchronize()
    return res, kc, vc


@pytest.mark.parametrize("form", ["bf16", "f32", "x3"])
def test_table_aware_attention_is_the_plain_attention_on_a_gathered_cache(form):
    dtype = torch.bfloat16 if form == "bf16" else torch.float32
    for pos in (0, 37, 300):
        Tmax = 48 if pos < 48 else 320
        part, bias, kc, vc, keep, rows, posd, B, nH, Tmax, pos, splits = _attn_case(dtype, Tmax=Tmax, pos=pos, seed=pos)
        ident = torch.arange(B, dtype=torch.int32, device=DEV)[:, None].expand(B, Tmax).contiguous()
        ref, rk, rv = _run_attn(form, part, bias, kc, vc, keep, posd, B, nH, Tmax, splits)
        got, gk, gv = _run_attn(form, part, bias, kc, vc, keep, posd, B, nH, Tmax, splits, rows=ident)
        assert torch.equal(got, ref) and torch.equal(gk, rk) and torch.equal(gv, rv), pos
        # a random table: the plain form on the cache gathered by it in torch (the token's own slot is row b's either way)
        j = torch.arange(Tmax, device=DEV)
        kg = kc[rows.long(), :, j[None, :].expand(B, Tmax)].permute(0, 2, 1, 3).contiguous()
        vg = vc[rows.long(), :, j[None, :].expand(B, Tmax)].permute(0, 2, 1, 3).contiguous()
        ref, rk, _ = _run_attn(form, part, bias, kg, vg, keep, posd, B, nH, Tmax, splits)
        got, gk, _ = _run_attn(form, part, bias, kc, vc, keep, posd, B, nH, Tmax, splits, rows=rows)
        assert torch.equal(got, ref), pos
        assert torch.equal(gk[:, :, pos], rk[:, :, pos]) and torch.equal(gk[:, :, :pos], kc[:, :, :pos]), pos


def _select_reference(logits, seq, keep, rows, scores, pos, P, nb, V):
    """torch restatement of one beam selection step (BeamDecoder's definition) on host copies."""
    seq, keep, rows, scores = seq.clone(), keep.clone(), rows.clone(), scores.clone()
    B = seq.shape[0]
    j = pos + 1 - P
    if j > 1 and (j + 1) % SENT in (0, 1):
        seq[:, pos + 1] = 2 if (j + 1) % SENT == 0 else 1
        rows[:, pos + 1] = torch.arange(B, dtype=torch.int32)
        return seq, keep, rows, scores
    cands = []
    for b in range(B):
        p = b % nb
        if int(seq[b, pos]) == 0:
            c = [(0.0, 0)] + [(float("-inf"), 0)] * (nb - 1)
        else:
            x = O.process_logits(logits[b], seq[b, P:pos + 1], T, REP)[:V]
            lp = torch.log_softmax(x, -1)
            order = torch.sort(x, descending=True, stable=True).indices[:nb].tolist()
            c = [(float(lp[v]), v) for v in order]
        cands.append([(np.float32(scores[b].item()) + np.float32(l), p, k, v) for k, (l, v) in enumerate(c)])
    out_seq, out_keep, out_rows = seq.clone(), keep.clone(), rows.clone()
    for g in range(B // nb):
        allc = sorted([c for b in range(g * nb, (g + 1) * nb) for c in cands[b]], key=lambda c: (-float(c[0]), c[1], c[2]))[:nb]
        for r, (s, p, _, v) in enumerate(allc):
            b, src = g * nb + r, g * nb + p
            out_seq[b, :pos + 1] = seq[src, :pos + 1]
            out_keep[b, :pos + 1] = keep[src, :pos + 1]
            out_rows[b, :pos + 1] = rows[src, :pos + 1]
            out_seq[b, pos + 1] = v
            out_rows[b, pos + 1] = b
            scores[b] = float(s)
    return out_seq, out_keep, out_rows, scores


def test_selection_kernels_match_a_torch_restatement():
    """Crafted rows: exact logit ties inside a row and across beams (equal rows, equal scores), a PAD-sticky beam, -inf start
    beams, and forced positions.  Tokens, parents, the reordered seq / keep / table agree exactly; scores to fp32 rounding of
    the log-sum-exp (the kernel and torch sum the exponentials in different orders)."""
    nb, n, P, V, Vp, Tmax = 4, 3, 5, 160, 168, 64
    B = n * nb
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, Vp, generator=g) * 3
    logits[:, 20] = logits[:, 21] = logits[:, 22] = 9.0               # exact ties inside every row (ids 20 < 21 < 22)
    logits[9] = logits[8]                                             # prompt 2: beams 0 and 1 identical ...
    seq = torch.randint(30, 99, (B, Tmax), generator=g)              # (no history token among the tied ids: no penalty splits them)
    seq[:, P] = 1
    keep = torch.randint(0, 2, (B, Tmax), generator=g, dtype=torch.int32)
    rows = torch.randint(0, B, (B, Tmax), generator=g, dtype=torch.int32)
    scores = -torch.rand(B, generator=g) * 5
    scores[0:4] = torch.tensor([0.0, float("-inf"), float("-inf"), float("-inf")])   # prompt 0: the start of a search
    pos = P + 10
    seq[5, pos] = 0                                                   # prompt 1: a PAD-sticky beam ...
    scores[5] = -0.25                                                 # ... with the best score of its prompt
    seq[9, :pos + 1] = seq[8, :pos + 1]
    scores[9] = scores[8]                                             # ... with equal scores: the parent order decides
    for p_ in (pos, P + 20, P + 21, P + 42):                          # a model call, [#EOS#], [#START#], [#EOS#]
        d = [t.to(DEV) for t in (logits, seq, keep, rows, scores)]
        dl, ds, dk, dr, dsc = d
        cv = torch.zeros(B, nb, device=DEV)
        ci = torch.zeros(B, nb, dtype=torch.int32, device=DEV)
        posd = torch.tensor([p_, 0], dtype=torch.int32, device=DEV)
        hip.decode_beam_candidates(dl, Vp, V, ds, posd[0:1], P, SENT, T, REP, nb, cv, ci, B)
        hip.decode_beam_merge(cv, ci, dsc, ds, dk, dr, posd[0:1], P, SENT, nb, n, pos_next=posd[1:2])
        torch.cuda.synchronize()
        rs, rk, rr, rsc = _select_reference(logits, seq, keep, rows, scores, p_, P, nb, V)
        assert int(posd[1]) == p_ + 1
        assert torch.equal(ds.cpu(), rs), p_
        assert torch.equal(dk.cpu(), rk) and torch.equal(dr.cpu(), rr), p_
        got = dsc.cpu()
        assert torch.equal(torch.isinf(got), torch.isinf(rsc)), p_
        np.testing.assert_allclose(got.numpy(), rsc.numpy(), rtol=1e-6, atol=1e-6)
        if p_ == pos:
            assert rs[4, pos + 1] == 0 and rr[4, pos] == rows[5, pos]     # the PAD beam leads prompt 1
            assert rs[0:3, pos + 1].tolist() == [20, 21, 22]              # the start beam's exact ties, lowest id first


# ------------------------------------------------------------------ 7. full size: determinism and batch-order invariance
def test_full_size_beam_runs_are_bit_stable():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    n, nb, Ln = 64, 4, 220
    nbt = synth.make_batch(n, mcfg, dcfg, V, seed=11)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    dec = BeamDecoder(model, n, nb, max_len=Ln)
    assert dec.fused and dec.use_graph
    i1, s1 = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP)
    i2, s2 = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    ie, se = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP, use_graph=False)
    assert torch.equal(ie, i1) and torch.equal(se, s1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).to(DEV)
    ip, sp = dec.generate({k: v[perm] for k, v in batch.items()}, Ln, temperature=T, repitition_penalty=REP)
    assert torch.equal(ip, i1[perm]) and torch.equal(sp, s1[perm])
    assert torch.isfinite(s1).all() and (s1[:, :-1] >= s1[:, 1:]).all()
    assert int(i1.min()) >= 0 and int(i1.max()) < V and (i1[:, :, 0] == 1).all()


def test_generate_beams_texts():
    """generate_beams: at one beam every prompt's text is the reference's greedy text (postprocess.npz case 0 =
    greedy_len220_row0); with four beams and return_all, each prompt's (text, score) list is the decoder's beams cut and
    post-processed, best first; max_batch splits the prompts into chunks."""
    import json
    import os
    from helpers import GOLDEN
    from mmtg_amd.generate import generate_beams, postprocess_tokens
    model, tb = build("tiny_s5", "f32")
    pp = np.load(os.path.join(GOLDEN, "postprocess.npz"))
    vocab = {int(k): v for k, v in json.loads(str(pp["vocab_json"])).items()}
    expected = json.loads(str(pp["expected_json"]))

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [vocab.get(int(i), "tok%d" % int(i)) for i in ids]

    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    assert generate_beams(model, {k: v[:1] for k, v in rows.items()}, Tok(), num_beams=1, length=220)[0] == expected[0]
    allb = generate_beams(model, rows, Tok(), num_beams=4, length=66, return_all=True)
    ids, scores = BeamDecoder(model, 3, 4, max_len=66).generate(tb, 66, temperature=1.1, repitition_penalty=1.5)
    for r in range(3):
        want = [(postprocess_tokens(Tok().convert_ids_to_tokens(GreedyDecoder.reference_return(ids[r, k].tolist(), 66))),
                 float(scores[r, k])) for k in range(4)]
        assert allb[r] == want, r
    chunked = generate_beams(model, rows, Tok(), num_beams=4, length=66, max_batch=8)      # 2 prompts per chunk, the last one padded
    assert len(chunked) == 3 and all(isinstance(t, str) for t in chunked)
