"""The ring form of the grouped weight-gradient kernel (mmtg_wgrad_group config 8 = hip.WGRAD_RING; the engine's
MMTG_WGRAD_GROUP_CFG=2): 256x256 tiles, one 16-wave workgroup per CU over a ring of three 32-k stages.

Per output element it adds in config 0's order (k ascending inside a K slice, slices in split order), so for an equal split count
the bar is torch.equal against config 0; against the float64 product of the same bf16 operands the bound is the one
tests/test_ops_gpu.py holds config 0 to (2e-5 of the result's largest magnitude: fp32 summation order only).
"""
import numpy as np
import pytest
import torch

from helpers import rnd  # noqa: E402
from mmtg_amd import hip  # noqa: E402

DEV = "cuda"
RING = hip.WGRAD_RING

# K slices of exactly one ring turn more or less, and ragged last stages; (K, splits) pairs the engine's rule can produce
# (no slice under 1024 tokens) ...
RING_EDGES = [(1024, 1), (1056, 1), (2080, 1), (2080, 2), (2112, 1), (2112, 2)]
# ... and, given to the kernel directly, slices that end inside a 32-k stage (1000 = 31 stages + 8 rows; 2100 / 2 -> 1088 + 1012)
RAGGED_STAGE = [(1000, 1), (2100, 2)]


def test_split_rule_keeps_the_ring_edge_shapes():
    """(no GPU) the engine's rule on the ring form's 256 slots gives the split counts the ring-edge cases use, and the K slices
    they mean: whole numbers of 32-k stages around one ring turn (3 stages)."""
    from mmtg_amd.engine import _group_splits
    for K, want in ((1024, 1), (1056, 1), (2080, 2), (2112, 2)):
        assert _group_splits(4, K, 256) == want
    assert _group_splits(108, 15104, 256) == 2                  # a GPT-2 base block: 27 + 9 + 36 + 36 tiles, one round of the CUs
    assert hip.wgrad_group_sizes(((768, 3072), (3072, 768), (768, 768), (768, 2304)), 2, RING) == (108, 108 * 2 * 65536, 108 * 16)
    def stages(K, s):           # 32-k stages of every K slice (slices are whole 64-k units, the last one takes what is left)
        kper = -(-(-(-K // s)) // 64) * 64
        return [-(-min(kper, K - k0) // 32) for k0 in range(0, K, kper)]
    assert [stages(K, s) for K, s in RING_EDGES] == [[32], [33], [65], [34, 31], [66], [34, 32]]
    assert [stages(K, s) for K, s in RAGGED_STAGE] == [[32], [34, 32]] and 1000 % 32 and (2100 - 1088) % 32


def _operands(shapes, K, seed, pad=0):
    """[(A [K, lda] bf16, B [K, ldb] bf16, M, N, lda, ldb)] on the device."""
    ops = []
    for i, (M, N) in enumerate(shapes):
        lda, ldb = M + pad, N + pad
        ops.append((rnd(K, lda, dtype=torch.bfloat16, seed=seed + 2 * i).to(DEV), rnd(K, ldb, dtype=torch.bfloat16, seed=seed + 2 * i + 1).to(DEV),
                    M, N, lda, ldb))
    return ops


def _launch(config, ops, K, splits, accumulate=False, fill=7.0, cnt=None):
    shapes = [(M, N) for (_, _, M, N, _, _) in ops]
    _, nws, ncnt = hip.wgrad_group_sizes(shapes, splits, config)
    ws = torch.full((nws,), float("nan"), device=DEV)
    if cnt is None:
        cnt = torch.zeros(ncnt, dtype=torch.int32, device=DEV)
    Cs = [torch.full((M, N + 8), fill, device=DEV) for (M, N) in shapes]            # ldc = N + 8: the pad columns stay as they are
    hip.wgrad_group([(A, B, C_, M, N, lda, ldb, N + 8) for (A, B, M, N, lda, ldb), C_ in zip(ops, Cs)], K, splits, ws, cnt,
                    accumulate=accumulate, config=config)
    assert int(cnt.abs().sum()) == 0
    return Cs


def _check(ops, K, splits):
    """overwrite and accumulate: the ring form equals config 0 bit for bit and the float64 product within config 0's bound"""
    ring = _launch(RING, ops, K, splits)
    base = _launch(0, ops, K, splits)
    for (A, B, M, N, _, _), r, b in zip(ops, ring, base):
        assert torch.equal(r, b)
        assert (r[:, N:] == 7.0).all()
        ref = A[:, :M].double().t() @ B[:, :N].double()
        assert (r[:, :N].double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
    ring = _launch(RING, ops, K, splits, accumulate=True, fill=1.0)
    base = _launch(0, ops, K, splits, accumulate=True, fill=1.0)
    for (A, B, M, N, _, _), r, b in zip(ops, ring, base):
        assert torch.equal(r, b)
        assert (r[:, N:] == 1.0).all()
        ref = A[:, :M].double().t() @ B[:, :N].double()
        assert (r[:, :N].double() - 1.0 - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("K,splits", RING_EDGES + RAGGED_STAGE)
def test_ring_edges(K, splits):
    _check(_operands([(256, 256), (264, 520)], K, seed=K + splits), K, splits)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(256, 256), (768, 64), (264, 520)])      # one full tile; padded column tiles; ragged both ways
@pytest.mark.parametrize("K,splits", [(2080, 2), (1056, 1)])
def test_tile_edges(shape, K, splits):
    _check(_operands([shape], K, seed=11), K, splits)


@pytest.mark.gpu
@pytest.mark.parametrize("K,splits", [(2112, 2), (1024, 1)])
def test_grouped_launch_of_four_problems(K, splits):
    """small analogues of a block's D x 3D, D x D, D x 4D and 4D x D gradients (D = 128), leading dimensions wider than the extents"""
    D = 128
    _check(_operands([(D, 3 * D), (D, D), (D, 4 * D), (4 * D, D)], K, seed=21, pad=8), K, splits)


@pytest.mark.gpu
def test_ragged_k_never_reads_past_the_operands():
    """NaN-filled memory directly behind both operands (same allocation): rows at or past the end of a K slice must be requested
    out of range per lane, also by the ring's requests two stages past the slice."""
    K, M, N = 1000, 384, 264
    bufA = torch.full((K + 256, M), float("nan"), dtype=torch.bfloat16, device=DEV)
    bufB = torch.full((K + 256, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    bufA[:K] = rnd(K, M, dtype=torch.bfloat16, seed=3).to(DEV)
    bufB[:K] = rnd(K, N, dtype=torch.bfloat16, seed=4).to(DEV)
    for splits in (1, 3):
        (C_,) = _launch(RING, [(bufA[:K], bufB[:K], M, N, M, N)], K, splits)
        ref = bufA[:K].double().t() @ bufB[:K].double()
        assert torch.isfinite(C_[:, :N]).all()
        assert (C_[:, :N].double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.gpu
def test_repeated_launches_are_bit_equal_and_leave_the_counters_zero():
    K, splits = 2080, 2
    ops = _operands([(768, 520), (264, 768)], K, seed=31)
    cnt = torch.zeros(hip.wgrad_group_sizes([(768, 520), (264, 768)], splits, RING)[2], dtype=torch.int32, device=DEV)
    first = _launch(RING, ops, K, splits, cnt=cnt)
    second = _launch(RING, ops, K, splits, cnt=cnt)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert int(cnt.abs().sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [2, 3])
def test_training_steps_equal_config_0_bit_for_bit(layers, monkeypatch):
    """Two training steps (V = 160, 12 rows, dropout 0.1) with the blocks' and the tied embedding's weight gradients on the ring form
    against the 128x128 form: the same split counts, so gradient buffer and parameters are equal bit for bit."""
    from mmtg_amd import MMTG, engine as E, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.trainer import MMTGTrainer
    S, V = 5, 160
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    gcfg = gpt2_config(n_layer=layers, vocab_size=V, n_positions=256, embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1)
    weights = synth.make_weights(mcfg, gcfg, seed=100)
    batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in synth.make_batch(12, mcfg, dcfg, V, seed=7).items()}
    results, launches = {}, {}
    orig = E.hip.wgrad_group
    for cfg in (0, 2):
        monkeypatch.setattr(E, "_WGRAD_GROUP_CFG", cfg)
        model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, token_table=synth.make_token_table(V, seed=101), compute_dtype="bf16")
        model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
        model.to(DEV).train()
        tr = MMTGTrainer(model, lr=1e-3, alpha=0.2)
        tr.eng.drop_seed = 4242
        seen = launches[cfg] = []

        def spy(probs, K, splits, *a, **k):
            seen.append((len(probs), splits, k.get("config", 0)))
            return orig(probs, K, splits, *a, **k)

        monkeypatch.setattr(E.hip, "wgrad_group", spy)
        tr.step(batch, stage=1)
        g = tr.eng.grad.detach().clone()
        tr.step(batch, stage=3)
        torch.cuda.synchronize()
        monkeypatch.setattr(E.hip, "wgrad_group", orig)
        results[cfg] = (g, model.engine().master.detach().clone())
    # the ring form really ran, for the blocks and for the tied embedding, at config 0's split counts
    assert len(launches[2]) == len(launches[0]) == 2 * (layers + 1)
    assert all(c == RING for (_, _, c) in launches[2]) and all(c == 0 for (_, _, c) in launches[0])
    assert [(n, s) for (n, s, _) in launches[2]] == [(n, s) for (n, s, _) in launches[0]]
    assert torch.equal(results[0][0], results[2][0])
    assert torch.equal(results[0][1], results[2][1])
    assert float(results[0][0].abs().max()) > 0
