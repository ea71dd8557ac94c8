#!/usr/bin/env python3
"""The price of the token-level unlikelihood term (MMTGTrainer(ul_weight=...)) at the full bf16 configuration (64 x 236, dropout on).

Two trainers on ONE model -- they share its engine, so the step is the same launches on the same buffers -- one with ul_weight=0.5
and one without, timed in one process as alternating blocks (without, with, without, with, ...).  A measurement is one event pair
around STEPS real optimizer steps (lr 1e-5) and one synchronise after it.  Then the new kernels alone between events, on the logits of
one forward: the term's forward (hip.loss_ul_fwd: the row kernel and the single-workgroup sample kernel), and the backward that carries
the term (hip.loss_bwd_ul) next to today's (hip.loss_bwd), both from the bf16 logits into a second bf16 buffer so that the logits
survive the repetitions (the trainer's launch writes in place: the same traffic).

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
W = 0.5
if not torch.cuda.is_available():
    sys.exit("bench_ul: needs the MI355X (a timing on the host says nothing)")
mcfg, dcfg, gcfg = make_model_cfgs(), data_config(), gpt2_config(vocab_size=V)
model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
model.reset_parameters(seed=0)
model.to(DEV).train()
trainers = {"plain": MMTGTrainer(model, lr=1e-5, alpha=0.2), "ul": MMTGTrainer(model, lr=1e-5, alpha=0.2, ul_weight=W)}
batches = [{n: torch.from_numpy(np.asarray(v)).to(DEV) for n, v in synth.make_batch(B, mcfg, dcfg, V, seed=s).items()} for s in range(4)]
T = int(batches[0]["targets"].shape[1]) + int(batches[0]["topic_ids"].shape[1])
eng = trainers["ul"].eng


def block(name):
    tr = trainers[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(STEPS):
        out = tr.step(batches[i % len(batches)], stage=3)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS, out


def kernel_ms(launch, reps=20, per=5):
    """median and minimum over `reps` event pairs around `per` back-to-back launches each, per launch"""
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


for name in trainers:                   # warm-up: workspaces, the moments
    block(name), block(name)
ms = {name: [] for name in trainers}
last = {}
for _ in range(ROUNDS):
    for name in ("plain", "ul"):
        t, last[name] = block(name)
        ms[name].append(t)
ul_value = float(last["ul"]["ul"])

# the kernels alone, on one forward's logits
batch = batches[0]
eng.forward(batch, train_flag=True, training=True, logits_f32=False)
eng.loss(batch["rating"], 3, batch_den=B)
eng.ul_loss(batch_den=B)
a, sh, Vp = eng.act, eng.sh, eng.layout.Vpad
M, L = a["M"], a["L"]
out = torch.empty(M, Vp, device=DEV, dtype=torch.bfloat16)
u = W / (L - 1)
fwd = lambda: hip.loss_ul_fwd(a["logits"], Vp, sh.V, a["targets"], a["lse_rows"], eng.ul_exclude, B, sh.P, L, float(B),
                              a["ul_row"], a["ul_S"], a["ul_sample"], a["ul"])
bwd_ul = lambda: hip.loss_bwd_ul(a["logits"], Vp, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"], float(B), a["ul_S"], u,
                                 eng.ul_exclude, B, sh.P, L, out, Vp, Vp)
bwd = lambda: hip.loss_bwd(a["logits"], Vp, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"], float(B), B, sh.P, L, out, Vp, Vp)
for f in (fwd, bwd_ul, bwd):
    for _ in range(3):
        f()
fwd_ms, fwd_min = kernel_ms(fwd)
bwd_ul_ms, bwd_ul_min = kernel_ms(bwd_ul)
bwd_ms, bwd_min = kernel_ms(bwd)
cands = float((a["ul_S"] > 0).sum())

med = {name: statistics.median(v) for name, v in ms.items()}
diff = [x - y for x, y in zip(ms["ul"], ms["plain"])]
print("unlikelihood term at the full bf16 configuration: %d rows x %d positions, dropout on; %d alternating rounds of %d steps, "
      "milliseconds per step" % (B, T, ROUNDS, STEPS))
for name in ("plain", "ul"):
    print("%-5s  median %7.3f  mean %7.3f  min %7.3f  max %7.3f   %9.0f tokens/s (median)" % (
        name, med[name], statistics.mean(ms[name]), min(ms[name]), max(ms[name]), 1e3 * B * T / med[name]))
print("ul - plain per round: median %+7.3f  min %+7.3f  max %+7.3f  (%.2f %% of the plain step); ul of the last step %.4f" % (
    statistics.median(diff), min(diff), max(diff), 100.0 * statistics.median(diff) / med["plain"], ul_value))
print("forward of the term alone (row + sample kernels): median %.4f ms (min %.4f), %d rows with candidates" % (fwd_ms, fwd_min, cands))
gb = 4.0 * M * Vp * 1e-6
print("backward with the term alone: median %.4f ms (min %.4f) = %.0f GB/s;  today's backward: median %.4f ms (min %.4f) = %.0f GB/s "
      "(bf16 in, bf16 out, %d x %d)" % (bwd_ul_ms, bwd_ul_min, gb / bwd_ul_ms, bwd_ms, bwd_min, gb / bwd_ms, M, Vp))
print(json.dumps({
    "tool": "bench_ul", "rows": B, "positions": T, "rounds": ROUNDS, "steps_per_block": STEPS, "ul_weight": W,
    "step_ms_plain": round(med["plain"], 4), "step_ms_ul": round(med["ul"], 4),
    "step_ms_diff_median": round(statistics.median(diff), 4), "step_ms_diff_min": round(min(diff), 4), "step_ms_diff_max": round(max(diff), 4),
    "step_cost_percent": round(100.0 * statistics.median(diff) / med["plain"], 3),
    "ul_fwd_ms": round(fwd_ms, 4), "loss_bwd_ul_ms": round(bwd_ul_ms, 4), "loss_bwd_ms": round(bwd_ms, 4),
    "loss_bwd_ul_gbps": round(gb / bwd_ul_ms, 1), "loss_bwd_gbps": round(gb / bwd_ms, 1),
    "ul": round(ul_value, 5), "finite": bool(torch.isfinite(eng.master).all())}))
