#!/usr/bin/env python3
"""The step tail (gradient norm + clip + AdamW + transposed-copy refresh: events around Engine.adamw_step) at the full bf16
configuration, three ways in one process, as alternating triples:

  plain      mmtg_sumsq + mmtg_adamw over the whole flat buffer (no param_groups)
  grouped    mmtg_sumsq_groups + mmtg_adamw_groups, everything trainable: the no_decay split, 116 segments
  frozen     the same entries with decoder.gpt2.* frozen

The gradients are those of one real training step; every timed call is a real update (lr 1e-5).  Prints per case the median, the
mean and the spread (min .. max) over the triples, and the per-triple differences grouped - plain.  ROUNDS=<n> (default 20)."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mmtg_amd import MMTG, hip, synth
from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
from mmtg_amd.param_groups import build_param_groups
from mmtg_amd.trainer import MMTGTrainer

DEV = "cuda"
ROUNDS = int(os.environ.get("ROUNDS", "20"))
V, B = 13317, int(os.environ.get("ROWS", "8"))
mcfg, dcfg, gcfg = make_model_cfgs(), data_config(), gpt2_config(vocab_size=V)
model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
model.reset_parameters(seed=0)
model.to(DEV).train()
tr = MMTGTrainer(model, lr=1e-5, alpha=0.2, weight_decay=0.1)
batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in synth.make_batch(B, mcfg, dcfg, V, seed=0).items()}
tr.step(batch, stage=3)                 # real gradients in eng.grad, moments allocated
eng = tr.eng
cases = {
    "plain": None,
    "grouped": hip.GroupTable(build_param_groups(eng.layout, [{"params": ["*bias*", "*ln_*"], "weight_decay": 0.0}], 0.1), DEV),
    "frozen": hip.GroupTable(build_param_groups(eng.layout, [{"params": "decoder.gpt2.*", "frozen": True}], 0.1), DEV),
}
count = torch.full((1,), float(B), device=DEV)


def tail(groups):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.adamw_step(1e-5, 1.0, (0.9, 0.999), 1e-6, 0.1, count=count, groups=groups)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1)


for g in cases.values():                # warm-up: every path twice
    tail(g), tail(g)
us = {k: [] for k in cases}
for _ in range(ROUNDS):
    for k, g in cases.items():
        us[k].append(tail(g))
n = eng.layout.total
print("step tail at the full bf16 configuration: %d parameters, %d keys; %d alternating triples, microseconds per tail" % (n, len(eng.layout.keys), ROUNDS))
for k, g in cases.items():
    seg = "" if g is None else " (%d segments, %d groups, %d trainable parameters)" % (
        g.nsegs, g.ngroups, sum(q["parameters"] for q in g.plan.groups if not q["frozen"]))
    print("%-8s median %8.1f  mean %8.1f  min %8.1f  max %8.1f%s" % (k, statistics.median(us[k]), statistics.mean(us[k]), min(us[k]), max(us[k]), seg))
for k in ("grouped", "frozen"):
    d = [a - b for a, b in zip(us[k], us["plain"])]
    print("%-8s - plain per triple: median %+8.1f  min %+8.1f  max %+8.1f" % (k, statistics.median(d), min(d), max(d)))
print("finite parameters:", bool(torch.isfinite(eng.master).all()))
