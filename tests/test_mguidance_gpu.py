"""Per-modality guidance on the MI355X: mmtg_decode_guidance_multi against the float64 restatement (constraints.modality_guidance_scores)
under the derived allowance of tests/mg_ref.py, in both forms and on both load paths; mmtg_decode_mirror_multi; generations of the
tiny model with two and three negatives against a host loop on the tapped logits; the structure of such a generation (the blocks on
one text, graph keys, scores, Mirostat) and the text surface.

Observed on an MI355X (docs/experiments.md has the table per (V, K)): the largest error of the kernel sweep is 0.29 of its allowance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mg_ref  # noqa: E402
from mmtg_amd import hip  # noqa: E402
from mmtg_amd.constraints import modality_guidance_scores  # noqa: E402
from mmtg_amd.decode import GreedyDecoder, GuidedDecoder, ModalityGuidedDecoder  # noqa: E402
from mmtg_amd.generate import without_experience, without_images, without_texts  # noqa: E402
from oracle import mmtg_oracle as O  # noqa: E402
from test_beam_cpu import SENT  # noqa: E402
from test_guidance_gpu import ATOL, Tok, tiny  # noqa: E402
from test_prefix_cpu import REP, T  # noqa: E402

DEV = "cuda"
SENTINEL = -77.0
OBSERVED = {}           # (V, K) -> (largest error, its allowance), printed by every case of the sweep


def negatives(tb, branches):
    """The negatives of `branches` for the device batch tb, as generate_samples builds them"""
    make = {"u": without_experience, "i": without_images, "t": without_texts}
    host = {k: v.cpu().numpy() for k, v in tb.items()}
    return [{k: v.to(DEV) for k, v in make[b](host).items()} for b in branches]


# ------------------------------------------------------------------ 1. the kernel against float64
def run_kernel(x, ld, scales, form, N):
    """The launch on mg_ref.padded(x, ld) into the middle rows of a sentinel-filled buffer whose rows are ld + 4 apart (so as aligned,
    or as odd, as the inputs'): returns the whole buffer [N + 2, ld + 4] on the host."""
    dev = torch.from_numpy(mg_ref.padded(x, ld)).to(DEV)
    buf = torch.full((N + 2, ld + 4), SENTINEL, device=DEV)
    hip.decode_guidance_multi(dev, ld, x.shape[2], scales, buf[1:N + 1], N, form=form)
    return buf.cpu().numpy()


def check_against_float64(V, K, N, ld, form):
    x = mg_ref.case(V, K, N)
    worst = (0.0, 1.0)
    for scales in mg_ref.SCALE_SETS[K]:
        want, allow = mg_ref.reference(V, K, N, scales)
        got = run_kernel(x, ld, scales, form, N)
        assert (got[0] == SENTINEL).all() and (got[N + 1] == SENTINEL).all() and (got[1:N + 1, V:] == SENTINEL).all()
        assert np.array_equal(got, run_kernel(x, ld, scales, form, N))          # equal inputs, equal bits
        g = got[1:N + 1, :V].astype(np.float64)
        fin = np.isfinite(want)
        assert not np.isnan(g).any() and np.array_equal(np.isfinite(g), fin) and bool(np.isneginf(g[~fin]).all())
        for b in range(N):
            if fin[b].any():
                err = float(np.abs(g[b][fin[b]] - want[b][fin[b]]).max())
                if err / allow[b] > worst[0] / worst[1]:
                    worst = (err, float(allow[b]))
                assert err <= allow[b], (V, K, N, ld, form, scales, b, err, allow[b])
        if all(s == 1.0 for s in scales):                                       # every scale at 1: lc, whatever the other rows hold
            lc = torch.log_softmax(torch.from_numpy(x[0].astype(np.float64)), -1).numpy()
            assert np.abs(g[fin] - lc[fin]).max() <= allow.max()
        if K == 2:                                                              # the two-row kernel on the same rows
            dev = torch.from_numpy(mg_ref.padded(x, ld)).to(DEV)
            two = torch.full((N, ld + 4), SENTINEL, device=DEV)
            hip.decode_guidance(dev, dev[N:], ld, V, scales[0], two, N)
            t = two.cpu().numpy()[:, :V].astype(np.float64)
            assert np.array_equal(np.isfinite(t), fin)
            for b in range(N):
                if fin[b].any():
                    assert np.abs(g[b][fin[b]] - t[b][fin[b]]).max() <= allow[b], (V, N, ld, form, scales, b)
    key = (V, K)
    if key not in OBSERVED or worst[0] / worst[1] > OBSERVED[key][0] / OBSERVED[key][1]:
        OBSERVED[key] = worst
    print("V %d K %d N %d ld %d %s: largest error %.3g, allowance %.3g (%.3f of it); (V, K) so far %.3g of %.3g"
          % (V, K, N, ld, form, worst[0], worst[1], worst[0] / worst[1], OBSERVED[key][0], OBSERVED[key][1]))


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("V", mg_ref.VS)
def test_the_kernel_against_float64_in_both_forms_on_both_load_paths(V, K, N):
    """mg_ref.case: normal times 4 with a +60 / -60 outlier, a -inf id in branch 1 only, with N = 3 an all -inf row in the last branch;
    input columns >= V hold 1e4; `out` is sentinel-filled with guard rows and wider than V.  The aligned stride takes the float4
    path, the odd one the one-logit path; "auto" is the register-resident form at these V, "reread" the two-pass one."""
    for ld in (mg_ref.aligned_ld(V), mg_ref.odd_ld(V)):
        for form in ("auto", "reread"):
            check_against_float64(V, K, N, ld, form)


@pytest.mark.parametrize("V", [14336, 14337])
def test_the_largest_v_the_registers_hold_and_the_first_beyond(V):
    """V = 14336 fills every register slot of the resident form on either path; at 14337 "auto" is the re-read form and "resident"
    is refused."""
    for ld in (mg_ref.aligned_ld(V), mg_ref.odd_ld(V)):
        check_against_float64(V, 4, 1, ld, "auto")
    x = mg_ref.case(V, 4, 1)
    if V > 14336:
        with pytest.raises(RuntimeError, match="14336"):
            run_kernel(x, mg_ref.aligned_ld(V), (3.0, 1.5, 0.5), "resident", 1)
        assert np.array_equal(run_kernel(x, mg_ref.aligned_ld(V), (3.0, 1.5, 0.5), "auto", 1),
                              run_kernel(x, mg_ref.aligned_ld(V), (3.0, 1.5, 0.5), "reread", 1))
    else:
        assert np.array_equal(run_kernel(x, mg_ref.aligned_ld(V), (3.0, 1.5, 0.5), "auto", 1),
                              run_kernel(x, mg_ref.aligned_ld(V), (3.0, 1.5, 0.5), "resident", 1))


def test_a_branch_equal_to_the_prompt_vanishes_bit_for_bit_on_the_device():
    V, N = 1025, 3
    x = np.array(mg_ref.case(V, 3, N))
    x[2] = x[0]                                                                 # the t branch is the prompt
    for ld in (mg_ref.aligned_ld(V), mg_ref.odd_ld(V)):
        for form in ("auto", "reread"):
            a = run_kernel(x, ld, (3.0, 0.0), form, N)
            b = run_kernel(x, ld, (3.0, 7.5), form, N)
            c = run_kernel(x[:2], ld, (3.0,), form, N)
            assert np.array_equal(a, b) and np.array_equal(a, c)


# ------------------------------------------------------------------ 2. the mirror
@pytest.mark.parametrize("N", [1, 3, 257])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_mirror_writes_one_column_of_the_later_blocks_and_nothing_else(K, N):
    ld = 37
    g = torch.Generator().manual_seed(100 * K + N)
    for col in (1, ld - 1, ld):
        seq = torch.randint(0, 1000, (K * N + 1, ld), generator=g) - 2000      # a sentinel range no id shares, a guard row behind
        seq[:N] = torch.randint(0, 1000, (N, ld), generator=g)
        dev = seq.to(DEV)
        pos = torch.tensor([col - 1], dtype=torch.int32, device=DEV)
        hip.decode_mirror_multi(dev, pos, N, K)
        want = seq.clone()
        if col < ld:
            for k in range(1, K):
                want[k * N:(k + 1) * N, col] = seq[:N, col]
        assert torch.equal(dev.cpu(), want) and int(pos.item()) == col - 1


# ------------------------------------------------------------------ 3. generation follows a host loop on the tapped logits
def follow_the_host_loop(dec, tb, branches, scales, length, **gen_kw):
    """A greedy generation with the negatives of `branches`, and for every step that called the head and every prompt: the float64 rule
    on the K tapped rows goes into the oracle's process_logits and gives the arg-max.  The device's pick must be it wherever the
    float64 top-2 gap exceeds twice the row's allowance (mg_ref.multi_allow of the K tapped rows; the processing divides every score
    by the penalty's powers and the temperature, both >= 1 here, so a score's error does not grow in it).  Returns (ids, checked,
    skipped)."""
    P, V, n, K = dec.eng.sh.P, min(dec.eng.sh.V, 13317), dec.n_prompts, dec.blocks
    steps = []

    def tap(j, with_head, picked, logits):
        if with_head:
            steps.append((j, picked.cpu().tolist(), logits[:, :V].float().cpu().numpy().copy(), dec.seq[:, P:P + j].cpu().tolist()))

    ids = dec.generate(tb, negatives(tb, branches), length, branches, scales, temperature=T, repitition_penalty=REP, tap=tap,
                       **gen_kw).cpu()
    checked = skipped = 0
    for j, picked, logits, hist in steps:
        assert logits.shape[0] == K * n
        x = logits.reshape(K, n, V)
        allow = mg_ref.multi_allow(x, scales)
        g = modality_guidance_scores(x, scales)
        for b in range(n):
            assert all(picked[k * n + b] == picked[b] and hist[k * n + b] == hist[b] for k in range(1, K))
            if hist[b][-1] == 0:
                assert picked[b] == 0
                continue
            top = torch.sort(O.process_logits(torch.from_numpy(g[b]), torch.tensor(hist[b]), T, REP), descending=True, stable=True)
            if not float(top.values[0] - top.values[1]) > 2 * allow[b]:
                skipped += 1
                continue
            assert picked[b] == int(top.indices[0]), (j, b)
            checked += 1
    return ids, checked, skipped


CASES = [(("i", "t"), (3.0, 1.5)), (("u", "i", "t"), (2.0, 3.0, 0.5))]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("branches,scales", CASES, ids=["two", "three"])
def test_greedy_generation_with_two_and_three_negatives_follows_the_host(mode, branches, scales):
    model, tb = tiny(mode)
    length = 3 * SENT
    dec = ModalityGuidedDecoder(model, 3, 1 + len(branches), max_len=length)
    ids, checked, skipped = follow_the_host_loop(dec, tb, branches, scales, length)
    print(mode, branches, scales, "checked", checked, "skipped", skipped)
    assert checked > 100 and 10 * skipped <= checked + skipped
    assert ids.shape == (3, 1 + length)
    plain = GreedyDecoder(model, 3, max_len=length).generate(tb, length, temperature=T, repitition_penalty=REP).cpu()
    assert not torch.equal(ids, plain)
    assert "3 prompts beside %d negatives each" % len(branches) in dec.describe() and "%s %g" % (branches[-1], scales[-1]) in dec.describe()


# ------------------------------------------------------------------ 4. structure
def test_every_block_stays_on_the_prompts_text_under_a_prefix_a_ban_bounds_and_a_refrain_at_once():
    model, tb = tiny("f32")
    length = 4 * SENT
    P = model.engine().sh.P
    line = [1, 7, 9, 11, 13]
    kw = dict(prefix=[line, line[:3], [1]], no_repeat_ngram_size=3, line_lengths=(2, 12), refrain_scheme="AB.A")
    for branches, scales in CASES:
        K = 1 + len(branches)
        dec = ModalityGuidedDecoder(model, 3, K, max_len=length)
        ids = dec.generate(tb, negatives(tb, branches), length, branches, scales, temperature=T, repitition_penalty=REP, **kw)
        cols = slice(P, P + 1 + length)
        for k in range(1, K):
            assert torch.equal(dec.seq[:3, cols], dec.seq[3 * k:3 * k + 3, cols])
        assert torch.equal(ids, dec.seq[:3, cols])
        for b, p in enumerate(kw["prefix"]):
            assert ids[b, :len(p)].tolist() == p
        eager = dec.generate(tb, negatives(tb, branches), length, branches, scales, temperature=T, repitition_penalty=REP,
                             use_graph=False, **kw)
        assert torch.equal(ids, eager)


def test_other_scales_capture_other_graphs_and_the_outputs_follow_their_own_scales():
    model, tb = tiny("f32")
    length = 2 * SENT
    branches = ("i", "t")
    dec = ModalityGuidedDecoder(model, 3, 3, max_len=length)
    a, checked_a, skipped_a = follow_the_host_loop(dec, tb, branches, (3.0, 1.5), length)
    keys_a = set(dec.graphs)
    b, checked_b, skipped_b = follow_the_host_loop(dec, tb, branches, (0.5, 7.5), length)      # the host loop holds each to its own scales
    new = set(dec.graphs) - keys_a
    assert keys_a and all(("modality_guidance", branches, (3.0, 1.5)) in k for k in keys_a)
    assert new and len(new) == len(keys_a) and all(("modality_guidance", branches, (0.5, 7.5)) in k for k in new)
    assert min(checked_a, checked_b) > 60 and 10 * skipped_a <= checked_a + skipped_a and 10 * skipped_b <= checked_b + skipped_b
    assert not torch.equal(a, b)
    fresh = ModalityGuidedDecoder(model, 3, 3, max_len=length)
    assert torch.equal(b, fresh.generate(tb, negatives(tb, branches), length, branches, (0.5, 7.5), temperature=T, repitition_penalty=REP).cpu())
    # the same scales on other branches are another key too
    dec.generate(tb, negatives(tb, ("u", "t")), length, ("u", "t"), (3.0, 1.5), temperature=T, repitition_penalty=REP)
    assert any(("modality_guidance", ("u", "t"), (3.0, 1.5)) in k for k in dec.graphs)


def test_scores_under_two_negatives_are_the_models_own_and_mirostat_moves_the_prompts_rows_only():
    from mmtg_amd.generate import score_sequences
    model, tb = tiny("f32")
    length = 2 * SENT
    branches, scales = ("i", "t"), (3.0, 1.5)
    dec = ModalityGuidedDecoder(model, 3, 3, max_len=length)
    gen = torch.Generator(device=DEV).manual_seed(9)
    ids, lp = dec.generate(tb, negatives(tb, branches), length, branches, scales, temperature=T, repitition_penalty=REP, top_k=0, top_p=0.0,
                           mirostat_tau=2.0, generator=gen, return_logprobs=True)
    mu = dec.mirostat_mu.cpu()
    assert bool((mu[3:] == 4.0).all()) and bool((mu[:3] != 4.0).all())
    assert lp.shape == ids.shape and bool((dec.tok_lp[3:] == 0).all())
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    want = score_sequences(model, rows, ids)
    np.testing.assert_allclose(lp.cpu().numpy(), want, atol=ATOL, rtol=0)
    assert float(np.abs(want).sum()) > 0


# ------------------------------------------------------------------ 5. the surface
def test_one_scale_alone_is_the_two_row_decoder_and_all_at_one_is_the_plain_call():
    from mmtg_amd.generate import generate_samples
    model, tb = tiny("f32")
    rows = {k: v.cpu().numpy() for k, v in tb.items()}
    gen = lambda: torch.Generator(device=DEV).manual_seed(4)
    kw = dict(n_samples=2, length=2 * SENT, line_lengths=7)
    P = model.engine().sh.P
    for name, make in (("image_guidance_scale", without_images), ("text_guidance_scale", without_texts)):
        one, two = GuidedDecoder(model, 6, max_len=2 * SENT), GuidedDecoder(model, 6, max_len=2 * SENT)
        a = generate_samples(model, rows, Tok(), generator=gen(), decoder=one, **{name: 3.0}, **kw)
        b = generate_samples(model, rows, Tok(), generator=gen(), decoder=two, guidance_scale=3.0, negative_rows=make(rows), **kw)
        assert one.graphs and two.graphs and set(one.graphs) == set(two.graphs)                # the decoder given, the two-row keys
        assert torch.equal(one.seq, two.seq) and a == b
    plain = generate_samples(model, rows, Tok(), generator=gen(), **kw)
    assert a != plain
    dec = GreedyDecoder(model, 6, max_len=2 * SENT)
    c = generate_samples(model, rows, Tok(), generator=gen(), decoder=dec, **kw)
    keys = set(dec.graphs)
    d = generate_samples(model, rows, Tok(), generator=gen(), decoder=dec, guidance_scale=1.0, image_guidance_scale=1.0,
                         text_guidance_scale=1.0, **kw)
    assert c == d == plain and set(dec.graphs) == keys
    # two scales: texts come back, one chunk of max_batch // 3 rows per generate
    mdec = ModalityGuidedDecoder(model, 2, 3, max_len=2 * SENT)
    texts = generate_samples(model, rows, Tok(), generator=gen(), decoder=mdec, max_batch=6, image_guidance_scale=3.0,
                             text_guidance_scale=1.5, **kw)
    assert mdec.graphs and len(texts) == 3 and all(len(t) == 2 and all(isinstance(s, str) and s for s in t) for t in texts)
    assert texts != plain and texts != a
    for t in texts:
        assert all(len(s.split("，")[0]) == 7 for s in t)
    scored = generate_samples(model, rows, Tok(), generator=gen(), decoder=mdec, max_batch=6, image_guidance_scale=3.0,
                              text_guidance_scale=1.5, return_scores=True, **kw)
    assert [[s for s, _, _ in t] for t in scored] == texts and all(np.isfinite(lp) and lp < 0 for t in scored for _, lp, _ in t)


def test_sample_sequence_with_two_scales_is_the_one_prompt_decoder():
    from mmtg_amd.generate import sample_sequence
    model, tb = tiny("f32")
    length = 2 * SENT
    start = {k: v[0].cpu().numpy() for k, v in tb.items()}
    start["targets"] = np.asarray([1])
    kw = dict(temperature=T, top_k=1, top_p=0.0, repitition_penalty=REP)
    got = sample_sequence(model, start, length, Tok(), image_guidance_scale=3.0, text_guidance_scale=1.5, **kw)
    one = {k: v[:1] for k, v in tb.items()}
    branches, scales = ("i", "t"), (3.0, 1.5)
    ids = ModalityGuidedDecoder(model, 1, 3, max_len=length).generate(one, negatives(one, branches), length, branches, scales,
                                                                     temperature=T, repitition_penalty=REP)
    assert got == GreedyDecoder.reference_return(ids[0].tolist(), length)
    assert got != sample_sequence(model, start, length, Tok(), **kw)
    three = sample_sequence(model, start, length, Tok(), guidance_scale=2.0, image_guidance_scale=3.0, text_guidance_scale=0.5, **kw)
    branches, scales = ("u", "i", "t"), (2.0, 3.0, 0.5)
    ids = ModalityGuidedDecoder(model, 1, 4, max_len=length).generate(one, negatives(one, branches), length, branches, scales,
                                                                     temperature=T, repitition_penalty=REP)
    assert three == GreedyDecoder.reference_return(ids[0].tolist(), length)
