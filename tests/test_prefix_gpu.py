"""Prefixed generation on the MI355X: GreedyDecoder / BeamDecoder with prefix=..., the *_fixed selection entries, and
generate_samples / generate_beams with prefixes=....  The decoder is held to the reference's own greedy output and to the CPU
restatements of tests/test_prefix_cpu.py."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GOLDEN  # noqa: E402
from mmtg_amd import hip  # noqa: E402
from mmtg_amd.decode import BeamDecoder, GreedyDecoder  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT, comparable_length, setup_case, start_row  # noqa: E402
from test_beam_gpu import build, full_size_model  # noqa: E402
from test_prefix_cpu import REP, T, cpu_prefixed_beam_search, cpu_prefixed_greedy, golden_prefix  # noqa: E402

DEV = "cuda"


def check_rules(ids, prefixes):
    """ids [B, 1 + length] (cpu): prefix columns untouched, cadence, no banned ids, sticky PAD after the prefix."""
    ids = ids.cpu()
    for b, p in enumerate(prefixes):
        L = len(p)
        assert ids[b, :L].tolist() == list(p), b
        for c in range(1, ids.shape[1]):
            v = int(ids[b, c])
            if c % SENT == SENT - 1:
                assert v == 2, (b, c)
            elif c % SENT == 0:
                assert v == 1, (b, c)
            else:
                assert v not in (1, 2, 100, 102), (b, c)
                if c >= L and int(ids[b, c - 1]) == 0:
                    assert v == 0, (b, c)


def mixed_prefixes(targets, rows):
    """Each row's own dataset lines, mixed lengths: [#START#] only, a partial line, 1, 2 and 4 lines (cycled over `rows`)."""
    kinds = [1, SENT + 5, SENT + 1, 2 * SENT + 1, 4 * SENT + 1]
    return [targets[r, :kinds[i % len(kinds)]].tolist() for i, r in enumerate(rows)]


# ------------------------------------------------------------------ 1. golden reproduction
@pytest.mark.parametrize("prefill", ["1", "0"])
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16x3f"])
def test_whole_line_prefix_cut_from_the_reference_output_gives_it_back(mode, prefill, monkeypatch):
    monkeypatch.setenv("MMTG_DECODE_PREFILL", prefill)
    fx = np.load(os.path.join(GOLDEN, "tiny_s5.npz"))
    model, tb = build("tiny_s5", mode)
    dec = GreedyDecoder(model, 3)
    assert dec.prefill == (prefill == "1")
    for k in (1, 3, 9):
        pre = [golden_prefix(fx, 0, k), golden_prefix(fx, 1, k), [1]]
        ids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, prefix=pre).cpu()
        if prefill == "1":
            assert dec.first_pos == model.engine().sh.P             # row 2's prefix is [#START#] alone: the prefill covers the prompt
        for row in (0, 1):
            assert GreedyDecoder.reference_return(ids[row].tolist(), 220) == fx["greedy_len220_row%d" % row].tolist(), (k, row)
    # the same prefix on every row: the prefill covers it (first_pos moves), the output is unchanged
    pre = [golden_prefix(fx, 1, 3)] * 3
    ids = dec.generate(tb, 220, temperature=T, repitition_penalty=REP, prefix=pre).cpu()
    if prefill == "1":
        assert dec.first_pos == model.engine().sh.P + 3 * SENT
    assert GreedyDecoder.reference_return(ids[1].tolist(), 220) == fx["greedy_len220_row1"].tolist()


# ------------------------------------------------------------------ 2. ground-truth prefixes, mixed lengths
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_mixed_length_ground_truth_prefixes_follow_the_cpu_restatement(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    rows = [0, 1, 2, 0, 1]
    pre = mixed_prefixes(batch["targets"], rows)
    tb5 = {k: v[rows] for k, v in tb.items()}
    length = 110
    ids = GreedyDecoder(model, 5, max_len=length).generate(tb5, length, temperature=T, repitition_penalty=REP, prefix=pre).cpu()
    check_rules(ids, pre)
    for i, r in enumerate(rows):
        want = cpu_prefixed_greedy(w, sh, table, start_row(batch, r), pre[i], length)
        assert ids[i].tolist() == want, i


# ------------------------------------------------------------------ 3. row independence
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_each_row_of_a_mixed_batch_is_that_row_decoded_alone(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    rows = [0, 1, 2, 0, 1]
    pre = mixed_prefixes(batch["targets"], rows)
    tb5 = {k: v[rows] for k, v in tb.items()}
    length = 132
    ids = GreedyDecoder(model, 5, max_len=length).generate(tb5, length, temperature=T, repitition_penalty=REP, prefix=pre).cpu()
    check_rules(ids, pre)
    if mode == "bf16":
        return
    one = GreedyDecoder(model, 1, max_len=length)
    for i, r in enumerate(rows):
        alone = one.generate({k: v[r:r + 1] for k, v in tb.items()}, length, temperature=T, repitition_penalty=REP, prefix=[pre[i]]).cpu()
        assert torch.equal(alone[0], ids[i]), i


# ------------------------------------------------------------------ 4. sampling
def test_sampling_with_a_prefix():
    """Prefix columns are exact in every sampled row; the logits at the first free position (read through tap) are the oracle's for
    that prefix, processed with the prefix counted (a token repeated at penalty 1.5); top_k = 1 sampling equals greedy."""
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", "f32")
    p = batch["targets"][0, :SENT + 1].tolist()
    rep_tok = p[1]
    p = p + [rep_tok, rep_tok]                                    # a partial line repeating a token of the first line
    pre = [p, p, [1]]
    L = len(p)
    dec = GreedyDecoder(model, 3, max_len=88)
    seen = {}

    def tap(j, with_head, picked, logits):
        if j == L and with_head:
            seen["logits"] = logits[0, :sh.V].float().cpu().clone()
            seen["picked"] = int(picked[0])

    g = torch.Generator(device=DEV).manual_seed(7)
    ids = dec.generate(tb, 88, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, generator=g, prefix=pre, tap=tap).cpu()
    check_rules(ids, pre)
    g = torch.Generator(device=DEV).manual_seed(7)
    again = dec.generate(tb, 88, temperature=T, repitition_penalty=REP, top_k=10, top_p=0.7, generator=g, prefix=pre).cpu()
    assert torch.equal(ids, again)
    cf = O.CachedForward(w, sh, table)
    base = {k: torch.as_tensor(np.asarray(v)).float().unsqueeze(0) for k, v in start_row(batch, 0).items()}
    base["topic_ids"] = base["topic_ids"].long()
    ref = cf(dict(base, targets=torch.tensor([p], dtype=torch.long)))[0, -1, :sh.V].float()
    np.testing.assert_allclose(seen["logits"].numpy(), ref.numpy(), rtol=0, atol=2e-3)
    counted = O.process_logits(seen["logits"].clone(), torch.tensor(p), T, REP)
    uncounted = O.process_logits(seen["logits"].clone(), torch.tensor([1]), T, REP)
    assert float(counted[rep_tok]) != float(uncounted[rep_tok])    # the prefix's occurrences are penalised
    gdec = GreedyDecoder(model, 3, max_len=88)
    gseen = {}

    def gtap(j, with_head, picked, logits):
        if j == L and with_head:
            gseen["picked"] = int(picked[0])

    greedy = gdec.generate(tb, 88, temperature=T, repitition_penalty=REP, prefix=pre, tap=gtap).cpu()
    assert gseen["picked"] == int(torch.argmax(counted[:min(sh.V, 13317)]))
    top1 = dec.generate(tb, 88, temperature=T, repitition_penalty=REP, top_k=1, top_p=0.5,
                        generator=torch.Generator(device=DEV).manual_seed(3), prefix=pre).cpu()
    assert torch.equal(top1, greedy)


# ------------------------------------------------------------------ 5. beams
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_one_beam_with_a_prefix_is_the_greedy_decoder(mode):
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    pre = mixed_prefixes(batch["targets"], [0, 1, 2])
    greedy = GreedyDecoder(model, 3).generate(tb, 220, temperature=T, repitition_penalty=REP, prefix=pre)
    ids, scores = BeamDecoder(model, 3, 1).generate(tb, 220, temperature=T, repitition_penalty=REP, prefix=pre)
    assert torch.equal(ids[:, 0], greedy)
    assert torch.isfinite(scores).all() and (scores < 0).all()


def test_four_beams_with_a_prefix_follow_the_cpu_beam_search():
    nb, full = 4, 110
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", "f32")
    pre = [batch["targets"][0, :SENT + 1].tolist(), batch["targets"][1, :SENT + 4].tolist(), golden_prefix(fx, 1, 2)]
    lens = []
    for row in range(3):
        _, _, gaps = cpu_prefixed_beam_search(w, sh, table, start_row(batch, row), pre[row], full, nb)
        lens.append(comparable_length(gaps, full))
    assert max(lens) >= 60, lens
    dec = BeamDecoder(model, 3, nb, max_len=full)
    runs = {}
    for row, L in enumerate(lens):
        if L < len(pre[row]):
            continue
        if L not in runs:
            runs[L] = [t.cpu() for t in dec.generate(tb, L, temperature=T, repitition_penalty=REP, prefix=pre)]
        ids, scores = runs[L]
        cids, cscores, _ = cpu_prefixed_beam_search(w, sh, table, start_row(batch, row), pre[row], L, nb)
        assert ids[row].tolist() == cids.tolist(), (row, L)
        np.testing.assert_allclose(scores[row].numpy(), cscores, rtol=0, atol=1e-3)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_prefixed_beam_scores_rescore_through_teacher_forced_greedy_decoding(mode):
    """Every returned score is the sum of the fp32 log-probabilities of the processed logits at the FREE positions the beam's
    tokens were chosen at (teacher-forced through GreedyDecoder with the same prefix); prefix positions add nothing."""
    nb, length = 4, 100
    fx, sh, w, table, batch = setup_case("tiny_s5")
    model, tb = build("tiny_s5", mode)
    pre = mixed_prefixes(batch["targets"], [0, 1, 2])
    ids, scores = BeamDecoder(model, 3, nb, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP, prefix=pre)
    n = 3
    flat = ids.reshape(n * nb, -1).cpu()
    rpre = [p for p in pre for _ in range(nb)]
    acc = np.zeros(n * nb, np.float64)
    V = sh.V

    def tap(j, with_head, picked, logits):
        if not with_head:
            return
        lg = logits[:, :V].float().cpu()
        for r in range(n * nb):
            if j < len(rpre[r]):
                continue
            hist = flat[r, :j]
            if int(hist[-1]) == 0:
                continue
            x = O.process_logits(lg[r], hist, T, REP)[:min(V, 13317)]
            acc[r] += float(torch.log_softmax(x, -1)[int(flat[r, j])])

    rep = {k: v.repeat_interleave(nb, 0) for k, v in tb.items()}
    GreedyDecoder(model, n * nb, max_len=length).generate(rep, length, temperature=T, repitition_penalty=REP, teacher=flat, tap=tap,
                                                          prefix=rpre)
    np.testing.assert_allclose(acc.reshape(n, nb), scores.cpu().numpy().astype(np.float64), rtol=1e-3, atol=0)
    check_rules(flat, rpre)


# ------------------------------------------------------------------ 6. kernels
def test_fixed_selection_entries_match_the_plain_ones_on_free_rows():
    """Rows with fixed_end <= pos + 1: the *_fixed entries write bit for bit what the plain entries write.  Rows with
    fixed_end > pos + 1: seq (and the beam state) untouched.  pos_next is written either way."""
    B, P, V, Vp, Tmax, nb = 8, 5, 160, 168, 64, 4
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(B, Vp, generator=g) * 3).to(DEV)
    seq0 = torch.randint(3, 99, (B, Tmax), generator=g)
    seq0[:, P] = 1
    seq0 = seq0.to(DEV)
    keep0 = torch.randint(0, 2, (B, Tmax), generator=g, dtype=torch.int32).to(DEV)
    rows0 = torch.randint(0, B, (B, Tmax), generator=g, dtype=torch.int32).to(DEV)
    scores0 = (-torch.rand(B, generator=g) * 5).to(DEV)
    uni = torch.rand(Tmax, B, generator=g).clamp_(max=1 - 2.0 ** -24).to(DEV)
    for pos in (P + 10, P + 20, P + 21):                         # a model call, [#EOS#], [#START#]
        # rows 0, 1, 4-7 on a prefix column, rows 2 (fixed_end = pos + 1) and 3 free
        fe = torch.tensor([pos + 2, pos + 5, pos + 1, 0, pos + 2, pos + 2, pos + 2, pos + 2], dtype=torch.int32, device=DEV)
        fixed = (fe > pos + 1).cpu()
        for kind in ("select", "sample", "none"):
            a, b_ = seq0.clone(), seq0.clone()
            pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
            pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
            if kind == "select":
                hip.decode_select(logits, Vp, V, a, pa[0:1], P, SENT, T, REP, B, pos_next=pa[1:2])
                hip.decode_select_fixed(logits, Vp, V, b_, pb[0:1], P, SENT, T, REP, B, fe, pos_next=pb[1:2])
            elif kind == "sample":
                hip.decode_sample(logits, Vp, V, a, pa[0:1], P, SENT, T, REP, 10, 0.7, uni, B, pos_next=pa[1:2])
                hip.decode_sample_fixed(logits, Vp, V, b_, pb[0:1], P, SENT, T, REP, 10, 0.7, uni, B, fe, pos_next=pb[1:2])
            else:
                hip.decode_select(None, 0, 0, a, pa[0:1], P, SENT, T, REP, B, pos_next=pa[1:2])
                hip.decode_select_fixed(None, 0, 0, b_, pb[0:1], P, SENT, T, REP, B, fe, pos_next=pb[1:2])
            torch.cuda.synchronize()
            assert int(pb[1]) == pos + 1 == int(pa[1])
            a, b_ = a.cpu(), b_.cpu()
            assert torch.equal(b_[~fixed], a[~fixed]), (pos, kind)
            assert torch.equal(b_[fixed], seq0.cpu()[fixed]), (pos, kind)
        # beams: prompt 0 = rows 0-3 on a prefix column, prompt 1 = rows 4-7 free (fixed_end <= pos + 1)
        fe_b = torch.tensor([pos + 3] * 4 + [pos + 1] * 4, dtype=torch.int32, device=DEV)
        st_a = [t.clone() for t in (seq0, keep0, rows0, scores0)]
        st_b = [t.clone() for t in (seq0, keep0, rows0, scores0)]
        cva, cia = torch.full((B, nb), 7.0, device=DEV), torch.full((B, nb), 7, dtype=torch.int32, device=DEV)
        cvb, cib = cva.clone(), cia.clone()
        pa = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
        pb = torch.tensor([pos, -1], dtype=torch.int32, device=DEV)
        hip.decode_beam_candidates(logits, Vp, V, st_a[0], pa[0:1], P, SENT, T, REP, nb, cva, cia, B)
        hip.decode_beam_merge(cva, cia, st_a[3], st_a[0], st_a[1], st_a[2], pa[0:1], P, SENT, nb, 2, pos_next=pa[1:2])
        hip.decode_beam_candidates_fixed(logits, Vp, V, st_b[0], pb[0:1], P, SENT, T, REP, nb, cvb, cib, B, fe_b)
        cvb_snap, cib_snap = cvb.clone(), cib.clone()
        hip.decode_beam_merge_fixed(cvb, cib, st_b[3], st_b[0], st_b[1], st_b[2], pb[0:1], P, SENT, nb, 2, fe_b, pos_next=pb[1:2])
        torch.cuda.synchronize()
        assert int(pb[1]) == pos + 1 == int(pa[1])
        # candidates: free rows as the plain entry, fixed rows untouched
        assert torch.equal(cvb_snap[4:], cva[4:]) and torch.equal(cib_snap[4:], cia[4:]), pos
        assert (cvb_snap[:4] == 7.0).all() and (cib_snap[:4] == 7).all(), pos
        # merge: the free prompt as the plain entry; the fixed prompt keeps seq / keep / scores, rows[b, pos + 1] = b
        for ta, tb_ in zip(st_a, st_b):
            assert torch.equal(tb_[4:], ta[4:]), pos
        assert torch.equal(st_b[0][:4], seq0[:4]) and torch.equal(st_b[1][:4], keep0[:4]) and torch.equal(st_b[3][:4], scores0[:4])
        want_rows = rows0[:4].clone()
        want_rows[:, pos + 1] = torch.arange(4, dtype=torch.int32, device=DEV)
        assert torch.equal(st_b[2][:4], want_rows), pos


# ------------------------------------------------------------------ 7. full size
def test_full_size_prefixed_decode_is_bit_stable_and_row_independent():
    from mmtg_amd import synth
    model, mcfg, dcfg, V = full_size_model("bf16")
    B, Ln = 256, 220
    nbt = synth.make_batch(B, mcfg, dcfg, V, seed=13)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in nbt.items() if k not in ("rating", "targets")}
    tg = np.asarray(nbt["targets"])
    pre = [tg[b, :1 + SENT * (b % 6)].tolist() for b in range(B)]          # 0 .. 5 whole lines
    dec = GreedyDecoder(model, B, max_len=Ln)
    assert dec.fused and dec.use_graph
    i1 = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP, prefix=pre)
    ie = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP, prefix=pre, use_graph=False)
    assert torch.equal(ie, i1)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(4))
    ip = dec.generate({k: v[perm.to(DEV)] for k, v in batch.items()}, Ln, temperature=T, repitition_penalty=REP,
                      prefix=[pre[int(i)] for i in perm])
    assert torch.equal(ip, i1[perm.to(DEV)])
    check_rules(i1, pre)
    assert int(i1.min()) >= 0 and int(i1.max()) < V
    # no prefix afterwards: the plain launches and graphs again, as a fresh decoder computes
    plain = dec.generate(batch, Ln, temperature=T, repitition_penalty=REP)
    assert not dec.rules.prefix
    assert torch.equal(plain, GreedyDecoder(model, B, max_len=Ln).generate(batch, Ln, temperature=T, repitition_penalty=REP))


# ------------------------------------------------------------------ 8. text surface
def test_generate_samples_and_beams_with_prefixes_give_the_reference_text():
    from mmtg_amd.generate import generate_beams, generate_samples
    fx = np.load(os.path.join(GOLDEN, "tiny_s5.npz"))
    model, tb = build("tiny_s5", "f32")
    pp = np.load(os.path.join(GOLDEN, "postprocess.npz"))
    vocab = {int(k): v for k, v in json.loads(str(pp["vocab_json"])).items()}
    expected = json.loads(str(pp["expected_json"]))

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [vocab.get(int(i), "tok%d" % int(i)) for i in ids]

    rows = {k: v[:1].cpu().numpy() for k, v in tb.items()}
    for k in (1, 4):
        pre = [golden_prefix(fx, 0, k)]
        s = generate_samples(model, rows, Tok(), n_samples=2, length=220, top_k=1, top_p=0.0, prefixes=pre)
        assert s == [[expected[0], expected[0]]], k
        assert generate_beams(model, rows, Tok(), num_beams=1, length=220, prefixes=pre) == [expected[0]], k
    with pytest.raises(ValueError):
        generate_samples(model, rows, Tok(), n_samples=2, length=220, prefixes=[[1], [1]])
    with pytest.raises(ValueError):
        generate_beams(model, rows, Tok(), num_beams=2, length=220, prefixes=[[2]])
