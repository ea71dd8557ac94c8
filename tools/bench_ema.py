#!/usr/bin/env python3
"""The price of the weight average (MMTGTrainer(ema_decay=...)) at the full bf16 configuration (64 x 236, dropout on).

Two trainers on ONE model -- they share its engine, so the step is the same launches on the same buffers -- one with
ema_decay=0.999 and one without, timed in one process as alternating blocks (without, with, without, with, ...).  A measurement is
one event pair around STEPS real optimizer steps (lr 1e-5) and one synchronise after it.  Then the update kernel alone
(hip.ema_update over the whole flat buffer, the trainer's launch) between events, in milliseconds and achieved GB/s at the 12 bytes
per parameter it has to move (read p, read ema, write ema), and the clip + AdamW kernel the same way for comparison (hip.adamw alone,
30 bytes per parameter: p, g, m, v in, p, m, v out, the bf16 copy out).

Prints the two medians, the per-round differences and ONE JSON line.  ROUNDS=<n> (default 10, at least 5), STEPS=<steps per
block> (default 10), ROWS=<rows per batch> (default 64)."""
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mmtg_amd import MMTG, hip, synth
from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
from mmtg_amd.trainer import MMTGTrainer

DEV = "cuda"
ROUNDS = max(5, int(os.environ.get("ROUNDS", "10")))
STEPS = max(1, int(os.environ.get("STEPS", "10")))
V, B = 13317, int(os.environ.get("ROWS", "64"))
if not torch.cuda.is_available():
    sys.exit("bench_ema: needs the MI355X (a timing on the host says nothing)")
mcfg, dcfg, gcfg = make_model_cfgs(), data_config(), gpt2_config(vocab_size=V)
model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
model.reset_parameters(seed=0)
model.to(DEV).train()
trainers = {"plain": MMTGTrainer(model, lr=1e-5, alpha=0.2), "ema": MMTGTrainer(model, lr=1e-5, alpha=0.2, ema_decay=0.999)}
batches = [{n: torch.from_numpy(np.asarray(v)).to(DEV) for n, v in synth.make_batch(B, mcfg, dcfg, V, seed=s).items()} for s in range(4)]
T = int(batches[0]["targets"].shape[1]) + int(batches[0]["topic_ids"].shape[1])
eng = trainers["ema"].eng
N = eng.layout.total


def block(name):
    tr = trainers[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(STEPS):
        tr.step(batches[i % len(batches)], stage=3)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


def kernel_ms(launch, reps=20, per=5):
    """median and minimum over `reps` event pairs around `per` back-to-back launches each, per launch (the buffers, 0.4 GB and more,
    do not stay in the 256 MB cache from one launch to the next)"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            launch()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / per)
    return statistics.median(out), min(out)


for name in trainers:                   # warm-up: workspaces, the moments, the average's first copy
    block(name), block(name)
ms = {name: [] for name in trainers}
for _ in range(ROUNDS):
    for name in ("plain", "ema"):
        ms[name].append(block(name))
assert trainers["ema"].ema_updates == (2 + ROUNDS) * STEPS and eng.ema is not None

count = trainers["ema"]._count
for _ in range(3):
    hip.ema_update(eng.ema, eng.master, N, 1e-3, count=count)
ema_ms, ema_min = kernel_ms(lambda: hip.ema_update(eng.ema, eng.master, N, 1e-3, count=count))
# (lr 0: the kernel's traffic without moving the parameters; the moments do move, the timed steps are over)
adam_ms, adam_min = kernel_ms(lambda: hip.adamw(eng.master, eng.grad, eng.opt_m, eng.opt_v, eng.wc, N, 0.0, 0.9, 0.999, 1e-6, 0.0,
                                                eng.step_count, eng.normsq, 1.0, count=count))

med = {name: statistics.median(v) for name, v in ms.items()}
diff = [a - b for a, b in zip(ms["ema"], ms["plain"])]
print("weight average at the full bf16 configuration: %d rows x %d positions, dropout on; %d alternating rounds of %d steps, "
      "milliseconds per step" % (B, T, ROUNDS, STEPS))
for name in ("plain", "ema"):
    print("%-5s  median %7.3f  mean %7.3f  min %7.3f  max %7.3f   %9.0f tokens/s (median)" % (
        name, med[name], statistics.mean(ms[name]), min(ms[name]), max(ms[name]), 1e3 * B * T / med[name]))
print("ema - plain per round: median %+7.3f  min %+7.3f  max %+7.3f  (%.2f %% of the plain step)" % (
    statistics.median(diff), min(diff), max(diff), 100.0 * statistics.median(diff) / med["plain"]))
print("update kernel alone: median %.3f ms (min %.3f) over %d parameters = %.0f GB/s at 12 B per parameter" % (
    ema_ms, ema_min, N, 12.0 * N / ema_ms * 1e-6))
print("clip + AdamW kernel alone: median %.3f ms (min %.3f) = %.0f GB/s at 30 B per parameter" % (adam_ms, adam_min, 30.0 * N / adam_ms * 1e-6))
print(json.dumps({
    "tool": "bench_ema", "rows": B, "positions": T, "rounds": ROUNDS, "steps_per_block": STEPS, "parameters": N,
    "step_ms_plain": round(med["plain"], 4), "step_ms_ema": round(med["ema"], 4),
    "step_ms_diff_median": round(statistics.median(diff), 4), "step_ms_diff_min": round(min(diff), 4), "step_ms_diff_max": round(max(diff), 4),
    "step_cost_percent": round(100.0 * statistics.median(diff) / med["plain"], 3),
    "ema_kernel_ms": round(ema_ms, 4), "ema_kernel_gbps": round(12.0 * N / ema_ms * 1e-6, 1),
    "adamw_kernel_ms": round(adam_ms, 4), "adamw_kernel_gbps": round(30.0 * N / adam_ms * 1e-6, 1),
    "finite": bool(torch.isfinite(eng.master).all() and torch.isfinite(eng.ema).all())}))
