#!/usr/bin/env python3
"""The price of the distillation term at the full bf16 configuration (64 x 236, dropout on).

Three trainers on ONE student model -- they share its engine, so the step is the same launches on the same buffers -- one without the
term, one with distill_weight = 0.5 at scale 1 (one teacher forward per step) and one at scale 2 (two), the teacher a second model
of the same size with its own engine.  Timed in one process as interleaved blocks (plain, scale 1, scale 2, plain, ...).  A
measurement is one event pair around STEPS real optimizer steps (lr 1e-5) and one synchronise after it.  Then the two new entries
alone between events on the 15104 x 13317 bf16 logits of the student and of the teacher's two forwards: hip.distill_fwd with and
without the negative beside one-scale hip.guided_loss on the teacher's pair, and hip.loss_bwd_kd (out of place, bf16 -> bf16) with
and without the negative beside hip.loss_bwd on the same logits, each with the bytes it moves and the rate that makes.

Prints the medians, the per-round differences and ONE JSON line.  ROUNDS=<n> (default 10, at least 5), STEPS=<steps per block>
(default 10), ROWS=<rows per batch> (default 64)."""
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
    sys.exit("bench_kd: needs the MI355X (a timing on the host says nothing)")
mcfg, dcfg, gcfg = make_model_cfgs(), data_config(), gpt2_config(vocab_size=V)


def make(seed):
    m = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
    m.reset_parameters(seed=seed)
    return m.to(DEV)


model, teacher = make(0).train(), make(1).eval()
trainers = {"plain": MMTGTrainer(model, lr=1e-5, alpha=0.2),
            "kd_s1": MMTGTrainer(model, lr=1e-5, alpha=0.2, distill_weight=W, distill_teacher=teacher, distill_scale=1.0),
            "kd_s2": MMTGTrainer(model, lr=1e-5, alpha=0.2, distill_weight=W, distill_teacher=teacher, distill_scale=2.0)}
NAMES = list(trainers)
batches = [{n: torch.from_numpy(np.asarray(v)).to(DEV) for n, v in synth.make_batch(B, mcfg, dcfg, V, seed=s).items()} for s in range(4)]
T = int(batches[0]["targets"].shape[1]) + int(batches[0]["topic_ids"].shape[1])


def block(name):
    tr = trainers[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(STEPS):
        out = tr.step(batches[i % len(batches)], stage=3)
    e1.record()
    torch.cuda.synchronize()
    # (read here: the three trainers share the engine, and with it the buffer 'kd' is a view of)
    return e0.elapsed_time(e1) / STEPS, (float(out["kd"]) if "kd" in out else None)


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


for name in NAMES:                      # warm-up: workspaces, the moments
    block(name), block(name)
ms = {name: [] for name in NAMES}
last = {}
for _ in range(ROUNDS):
    for name in NAMES:
        t, last[name] = block(name)
        ms[name].append(t)

# the entries alone
batch = batches[0]
model.eval()
tr = trainers["kd_s2"]
eng = tr.eng
cond, lse_c, uncond, lse_u = tr._teacher_pass(batch, 3)
eng.forward(batch, train_flag=True, training=False, logits_f32=False)
eng.loss(batch["rating"], 3, batch_den=B)
a, sh, Vp = eng.act, eng.sh, eng.layout.Vpad
M, L, P = a["M"], a["L"], sh.P
x, lse = a["logits"], a["lse_rows"]
assert x.dtype == torch.bfloat16 and cond.dtype == torch.bfloat16
outs = [torch.empty(n, device=DEV) for n in (M, M, B, 1)]
nll, smp, ce = torch.empty(M, device=DEV), torch.empty(B, device=DEV), torch.empty(1, device=DEV)
dl = torch.empty(M, Vp, device=DEV, dtype=torch.bfloat16)
ldt = cond.stride(0)
wc = W / (L - 1)
head = (x, Vp, sh.V, a["topic_ids"], a["targets"], lse, a["coef"], float(B))
launches = {
    "distill_fwd_s2": lambda: hip.distill_fwd(x, Vp, cond, uncond, ldt, sh.V, lse, lse_c, lse_u, 2.0, B, P, L, float(B), *outs),
    "distill_fwd_s1": lambda: hip.distill_fwd(x, Vp, cond, None, ldt, sh.V, lse, lse_c, None, 1.0, B, P, L, float(B), *outs),
    "guided_loss_k1": lambda: hip.guided_loss(cond, uncond, ldt, sh.V, lse_c, lse_u, a["topic_ids"], a["targets"], [2.0], B, P, L, float(B), nll, smp, ce),
    "loss_bwd_kd_s2": lambda: hip.loss_bwd_kd(*head, cond, uncond, ldt, lse_c, lse_u, 2.0, outs[1], wc, B, P, L, dl, Vp, Vp),
    "loss_bwd_kd_s1": lambda: hip.loss_bwd_kd(*head, cond, None, ldt, lse_c, None, 1.0, outs[1], wc, B, P, L, dl, Vp, Vp),
    "loss_bwd": lambda: hip.loss_bwd(*head, B, P, L, dl, Vp, Vp),
}
rowsV = 2.0 * B * (L - 1) * sh.V                # bytes of one bf16 matrix's loss rows
wr = 2.0 * M * Vp                               # bytes of the bf16 d(logits)
moved = {"distill_fwd_s2": 3 * rowsV, "distill_fwd_s1": 2 * rowsV, "guided_loss_k1": 2 * rowsV, "loss_bwd_kd_s2": 3 * rowsV + wr,
         "loss_bwd_kd_s1": 2 * rowsV + wr, "loss_bwd": rowsV + wr}
kern = {}
for name, f in launches.items():
    for _ in range(3):
        f()
    med, lo = kernel_ms(f)
    kern[name] = {"ms": round(med, 4), "min_ms": round(lo, 4), "mbytes": round(moved[name] * 1e-6, 1), "tbytes_per_s": round(moved[name] / med * 1e-9, 3)}

med = {name: statistics.median(v) for name, v in ms.items()}
spread = {name: max(v) - min(v) for name, v in ms.items()}
print("the distillation term at the full bf16 configuration: %d rows x %d positions, dropout on; %d interleaved rounds of %d steps, "
      "milliseconds per step" % (B, T, ROUNDS, STEPS))
for name in NAMES:
    print("%-6s median %7.3f  mean %7.3f  min %7.3f  max %7.3f   %9.0f tokens/s (median)" % (
        name, med[name], statistics.mean(ms[name]), min(ms[name]), max(ms[name]), 1e3 * B * T / med[name]))
diffs = {}
for name in NAMES[1:]:
    d = [p - q for p, q in zip(ms[name], ms["plain"])]
    diffs[name] = d
    print("%s - plain per round: median %+7.3f  min %+7.3f  max %+7.3f  (%.1f %% of the plain step); kd of the last step %.4f" % (
        name, statistics.median(d), min(d), max(d), 100.0 * statistics.median(d) / med["plain"], last[name]))
print("the entries alone on %d x %d bf16 logits (%d loss rows), median ms (min), MB moved, TB/s:" % (M, sh.V, B * (L - 1)))
for name, k in kern.items():
    print("  %-15s %8.4f (%.4f)  %8.1f MB  %6.3f TB/s" % (name, k["ms"], k["min_ms"], k["mbytes"], k["tbytes_per_s"]))
print(json.dumps({
    "tool": "bench_kd", "rows": B, "positions": T, "rounds": ROUNDS, "steps_per_block": STEPS, "distill_weight": W,
    "step_ms": {n: round(med[n], 4) for n in NAMES}, "step_ms_spread": {n: round(spread[n], 4) for n in NAMES},
    "step_ms_diff_median": {n: round(statistics.median(d), 4) for n, d in diffs.items()},
    "step_ms_diff_min": {n: round(min(d), 4) for n, d in diffs.items()}, "step_ms_diff_max": {n: round(max(d), 4) for n, d in diffs.items()},
    "kernels": kern, "finite": bool(torch.isfinite(eng.master).all())}))
