"""Shared helpers for the parity tests: rebuild the exact weights / batch a
fixture was generated from (seeds live in the fixture's meta record)."""
import json
import math
import os

import numpy as np
import torch

from mmtg_amd import synth
from mmtg_amd.configs import data_config, make_model_cfgs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(fx["meta"]))
    mcfg = make_model_cfgs(seq_len=meta["S"], **meta.get("enc", {}))      # "enc": encoder types / depths of the variant fixtures
    gcfg = meta["gpt2_cfg"]
    dcfg = data_config(seq_len=meta["S"])
    weights = synth.make_weights(mcfg, gcfg, seed=meta["weight_seed"])
    table = synth.make_token_table(meta["V"], seed=meta["table_seed"])
    batch = synth.make_batch(meta["B"], mcfg, dcfg, meta["V"], seed=meta["batch_seed"])
    return fx, meta, mcfg, gcfg, dcfg, weights, table, batch


def batch_to_torch(batch, device="cpu"):
    return {k: torch.from_numpy(np.asarray(v)).to(device) for k, v in batch.items()}


def sample_like_fixture(a, idx):
    return np.asarray(a, np.float32).reshape(-1)[idx]


# ------------------------------------------------------------------ the per-kernel GPU tests' inputs and tolerances
def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * scale
    return x.to(dtype)


def tol(dtype, k=1):
    """(atol, rtol) for an output of O(1) magnitude reduced over k terms."""
    if dtype == torch.float32:
        return 2e-5 * max(1.0, math.sqrt(k) / 8), 2e-5
    return 1e-2 * max(1.0, math.sqrt(k) / 16), 1.2e-2


def close(got, ref, dtype, k=1, name="", scale=None):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    atol, rtol = tol(dtype, k)
    s = float(ref.abs().max()) if scale is None else scale
    atol *= max(s, 1e-6)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), "%s: %d/%d mismatches, max err %.3e (ref max %.3e, atol %.2e)" % (
        name, int(bad.sum()), bad.numel(), float(err.max()), s, atol)


def planes_of(x):
    """fp32 [rows, cols] on the device -> its (hi | lo) bf16 plane pair (mmtg_split_planes)."""
    from mmtg_amd import hip
    rows, cols = x.shape
    return hip.split_planes(x.contiguous(), rows, cols, hip.Planes.empty(rows, cols, x.device))
