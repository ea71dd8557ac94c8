#!/usr/bin/env python3
"""Gradient accumulation at the full bf16 configuration (64 x 236, dropout on): whole windows of k micro-steps for k in 1, 2, 4, 8,
all four in one process as alternating rounds (k = 1, 2, 4, 8, then again) on one model -- the trainers share its engine and are
all at a window boundary whenever the turn passes on.  A measurement is one event pair around 8 / k whole windows, i.e. the same
eight micro-steps for every k, and one synchronise after it: the start-up of the launch queue after a synchronise costs every k
the same.

Every timed window is a real update (lr 1e-5).  Prints per k the median, the mean and the spread (min .. max) of the milliseconds per
MICRO-step (time / 8) and the tokens per second, and the per-round differences to k = 1.  ROUNDS=<n> (default 10, at least
5), ROWS=<rows per micro-batch> (default 64)."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mmtg_amd import MMTG, synth
from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
from mmtg_amd.trainer import MMTGTrainer

DEV = "cuda"
ROUNDS = max(5, int(os.environ.get("ROUNDS", "10")))
KS = (1, 2, 4, 8)
V, B = 13317, int(os.environ.get("ROWS", "64"))
mcfg, dcfg, gcfg = make_model_cfgs(), data_config(), gpt2_config(vocab_size=V)
model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
model.reset_parameters(seed=0)
model.to(DEV).train()
trainers = {k: MMTGTrainer(model, lr=1e-5, alpha=0.2, accumulation_steps=k) for k in KS}
batches = [{n: torch.from_numpy(np.asarray(v)).to(DEV) for n, v in synth.make_batch(B, mcfg, dcfg, V, seed=s).items()} for s in range(max(KS))]
T = int(batches[0]["targets"].shape[1]) + int(batches[0]["topic_ids"].shape[1])


def window(k):
    tr, n = trainers[k], max(KS)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):                  # n / k whole windows
        tr.step(batches[i], stage=3)
    e1.record()
    torch.cuda.synchronize()
    assert tr.micro_step == 0 and tr.window["rows"] == k * B
    return e0.elapsed_time(e1) / n


for k in KS:                            # warm-up: every k twice (workspaces of both backward forms, the lazy zero list)
    window(k), window(k)
ms = {k: [] for k in KS}
for _ in range(ROUNDS):
    for k in KS:
        ms[k].append(window(k))
print("gradient accumulation at the full bf16 configuration: %d rows x %d positions per micro-step, dropout on; %d alternating rounds, "
      "milliseconds per micro-step (8 micro-steps = 8 / k windows per measurement)" % (B, T, ROUNDS))
for k in KS:
    med = statistics.median(ms[k])
    print("k = %d  median %7.3f  mean %7.3f  min %7.3f  max %7.3f   %9.0f tokens/s (median)   rows per optimizer step %4d" % (
        k, med, statistics.mean(ms[k]), min(ms[k]), max(ms[k]), 1e3 * B * T / med, k * B))
for k in KS[1:]:
    d = [a - b for a, b in zip(ms[k], ms[1])]
    print("k = %d - k = 1 per round: median %+7.3f  min %+7.3f  max %+7.3f" % (k, statistics.median(d), min(d), max(d)))
print("finite parameters:", bool(torch.isfinite(trainers[1].eng.master).all()), " loss of the last k = 8 window: %.4f" % float(trainers[8].window["loss"]))
