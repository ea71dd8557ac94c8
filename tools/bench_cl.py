#!/usr/bin/env python3
"""The price of the contrastive token loss (MMTGTrainer(cl_weight=...)) at the full bf16 configuration (64 x 236, dropout on).

Two trainers on ONE model -- they share its engine, so the step is the same launches on the same buffers -- one with cl_weight=0.5
and one without, timed in one process as alternating blocks (without, with, without, with, ...).  A measurement is one event pair
around STEPS real optimizer steps (lr 1e-5) and one synchronise after it.  Then the two entries alone between events, on the ln_f
output and the keep mask of one forward: hip.cl_fwd (the reciprocal, tile and sample kernels) and hip.cl_bwd into a bf16 buffer of
d_hf's shape (it adds in place: the buffer drifts, the work does not), next to the LM-head loss kernels hip.loss_fwd / hip.loss_bwd
on the same forward, and beside two floors: the bytes the kernels must move (hf once for the forward and twice for the backward plus
one read-modify-write of d_hf, at the 8 TB/s of HBM) and their matrix-core FLOPs at the bf16 dense peak (2.5 PFLOP/s).

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
W, MARGIN = 0.5, 0.5
HBM_BPS, BF16_PEAK = 8.0e12, 2.5e15
if not torch.cuda.is_available():
    sys.exit("bench_cl: needs the MI355X (a timing on the host says nothing)")
mcfg, dcfg, gcfg = make_model_cfgs(), data_config(), gpt2_config(vocab_size=V)
model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
model.reset_parameters(seed=0)
model.to(DEV).train()
trainers = {"plain": MMTGTrainer(model, lr=1e-5, alpha=0.2), "cl": MMTGTrainer(model, lr=1e-5, alpha=0.2, cl_weight=W, cl_margin=MARGIN)}
batches = [{n: torch.from_numpy(np.asarray(v)).to(DEV) for n, v in synth.make_batch(B, mcfg, dcfg, V, seed=s).items()} for s in range(4)]
T = int(batches[0]["targets"].shape[1]) + int(batches[0]["topic_ids"].shape[1])
eng = trainers["cl"].eng


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
    for name in ("plain", "cl"):
        t, last[name] = block(name)
        ms[name].append(t)
cl_value = float(last["cl"]["cl"])

# the entries alone, on one forward's states
batch = batches[0]
eng.forward(batch, train_flag=True, training=True, logits_f32=False)
eng.loss(batch["rating"], 3, batch_den=B)
eng.cl_loss(MARGIN, batch_den=B)
a, sh, Vp = eng.act, eng.sh, eng.layout.Vpad
M, L, D, P = a["M"], a["L"], sh.D, sh.P
kept = int((a["keep"][:, P:] != 0).sum())
dhf = (1e-3 * torch.randn(M, D, device=DEV)).to(torch.bfloat16)
dl = torch.empty(M, Vp, device=DEV, dtype=torch.bfloat16)
fwd = lambda: hip.cl_fwd(a["hf"], D, a["keep"], P + L, MARGIN, B, P, L, D, float(B), a["cl_rinv"], a["cl_row"], a["cl_sample"], a["cl"])
bwd = lambda: hip.cl_bwd(a["hf"], D, a["keep"], P + L, a["cl_rinv"], MARGIN, W, B, P, L, D, dhf, D)
lfwd = lambda: eng.loss(batch["rating"], 3, batch_den=B)
lbwd = lambda: hip.loss_bwd(a["logits"], Vp, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"], float(B), B, P, L, dl, Vp, Vp)
for f in (fwd, bwd, lfwd, lbwd):
    for _ in range(3):
        f()
fwd_ms, fwd_min = kernel_ms(fwd)
bwd_ms, bwd_min = kernel_ms(bwd)
lfwd_ms, _ = kernel_ms(lfwd)
lbwd_ms, _ = kernel_ms(lbwd)
rows = B * L
floor_bytes = {"fwd": 2.0 * rows * D, "bwd": 2.0 * 2.0 * rows * D + 2.0 * 2.0 * rows * D}
flops = {"fwd": 2.0 * B * L * L * D, "bwd": 4.0 * B * L * L * D}
floor = {k: (1e3 * floor_bytes[k] / HBM_BPS, 1e3 * flops[k] / BF16_PEAK) for k in flops}

med = {name: statistics.median(v) for name, v in ms.items()}
diff = [x - y for x, y in zip(ms["cl"], ms["plain"])]
print("contrastive token loss at the full bf16 configuration: %d rows x %d positions, dropout on; %d alternating rounds of %d steps, "
      "milliseconds per step" % (B, T, ROUNDS, STEPS))
for name in ("plain", "cl"):
    print("%-5s  median %7.3f  mean %7.3f  min %7.3f  max %7.3f   %9.0f tokens/s (median)" % (
        name, med[name], statistics.mean(ms[name]), min(ms[name]), max(ms[name]), 1e3 * B * T / med[name]))
print("cl - plain per round: median %+7.3f  min %+7.3f  max %+7.3f  (%.2f %% of the plain step); cl of the last step %.5f" % (
    statistics.median(diff), min(diff), max(diff), 100.0 * statistics.median(diff) / med["plain"], cl_value))
print("mmtg_cl_fwd alone: median %.4f ms (min %.4f); floors: %.4f ms for %.1f MB at 8 TB/s, %.4f ms for %.2f GFLOP at the bf16 peak" % (
    fwd_ms, fwd_min, floor["fwd"][0], floor_bytes["fwd"] * 1e-6, floor["fwd"][1], flops["fwd"] * 1e-9))
print("mmtg_cl_bwd alone: median %.4f ms (min %.4f); floors: %.4f ms for %.1f MB at 8 TB/s, %.4f ms for %.2f GFLOP at the bf16 peak" % (
    bwd_ms, bwd_min, floor["bwd"][0], floor_bytes["bwd"] * 1e-6, floor["bwd"][1], flops["bwd"] * 1e-9))
print("the LM-head loss kernels on the same forward: mmtg_loss_fwd %.4f ms, mmtg_loss_bwd %.4f ms; the two new entries are %.2f of their sum "
      "(%d x %d lyric rows, %d kept, D = %d)" % (lfwd_ms, lbwd_ms, (fwd_ms + bwd_ms) / (lfwd_ms + lbwd_ms), B, L, kept, D))
print(json.dumps({
    "tool": "bench_cl", "rows": B, "positions": T, "rounds": ROUNDS, "steps_per_block": STEPS, "cl_weight": W, "cl_margin": MARGIN,
    "step_ms_plain": round(med["plain"], 4), "step_ms_cl": round(med["cl"], 4),
    "step_ms_diff_median": round(statistics.median(diff), 4), "step_ms_diff_min": round(min(diff), 4), "step_ms_diff_max": round(max(diff), 4),
    "step_cost_percent": round(100.0 * statistics.median(diff) / med["plain"], 3),
    "cl_fwd_ms": round(fwd_ms, 4), "cl_bwd_ms": round(bwd_ms, 4), "loss_fwd_ms": round(lfwd_ms, 4), "loss_bwd_ms": round(lbwd_ms, 4),
    "cl_fwd_floor_bytes_ms": round(floor["fwd"][0], 5), "cl_fwd_floor_flops_ms": round(floor["fwd"][1], 5),
    "cl_bwd_floor_bytes_ms": round(floor["bwd"][0], 5), "cl_bwd_floor_flops_ms": round(floor["bwd"][1], 5),
    "cl": round(cl_value, 5), "finite": bool(torch.isfinite(eng.master).all())}))
