#!/usr/bin/env python3
"""The price of the training side of guidance at the full bf16 configuration (64 x 236, dropout on).

Two trainers on ONE model -- they share its engine, so the step is the same launches on the same buffers -- one with
experience_drop=0.1 and one without, timed in one process as alternating blocks (without, with, without, with, ...).  A measurement
is one event pair around STEPS real optimizer steps (lr 1e-5) and one synchronise after it.  Then the two entries alone between
events: hip.experience_drop on the batch's two fp32 channels into bf16 buffers, beside the two hip.cast_f32_to launches it
replaces; and hip.guided_loss on the bf16 logits of two forwards (the batch, and the batch without its experience) with K = 1 and
K = 8 scales, next to hip.loss_fwd on the same logits and beside the floor of its bytes (both matrices' loss rows once, at the
8 TB/s of HBM).

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
PDROP = 0.1
SCALES8 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 7.5]
HBM_BPS = 8.0e12
if not torch.cuda.is_available():
    sys.exit("bench_cfg: needs the MI355X (a timing on the host says nothing)")
mcfg, dcfg, gcfg = make_model_cfgs(), data_config(), gpt2_config(vocab_size=V)
model = MMTG(mcfg, dcfg, V, train_flag=True, gpt2_config=gcfg, compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
model.reset_parameters(seed=0)
model.to(DEV).train()
trainers = {"plain": MMTGTrainer(model, lr=1e-5, alpha=0.2), "drop": MMTGTrainer(model, lr=1e-5, alpha=0.2, experience_drop=PDROP)}
batches = [{n: torch.from_numpy(np.asarray(v)).to(DEV) for n, v in synth.make_batch(B, mcfg, dcfg, V, seed=s).items()} for s in range(4)]
T = int(batches[0]["targets"].shape[1]) + int(batches[0]["topic_ids"].shape[1])
eng = trainers["drop"].eng


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
    for name in ("plain", "drop"):
        t, last[name] = block(name)
        ms[name].append(t)
dropped = int((last["drop"]["experience_drop"] != 0).sum())

# the entries alone
batch = batches[0]
S, E = int(batch["img_embs"].shape[1]), int(batch["img_embs"].shape[2])
n = S * E
img, txt = batch["img_embs"].to(DEV, torch.float32).contiguous(), batch["r_embs"].to(DEV, torch.float32).contiguous()
oi, ot = torch.empty(B * n, device=DEV, dtype=torch.bfloat16), torch.empty(B * n, device=DEV, dtype=torch.bfloat16)
code = torch.empty(B, device=DEV, dtype=torch.int32)
thr = hip.drop_thresholds((PDROP, 0.0, 0.0))
drop = lambda: hip.experience_drop(img, txt, oi, ot, code, B, n, 12345, thr)
casts = lambda: (hip.cast_f32_to(img, oi, B * n), hip.cast_f32_to(txt, ot, B * n))
model.eval()
ev = trainers["plain"].evaluate_guided_batch(batch, [1.0])              # leaves both logits matrices and their lse in place
a, sh, Vp = eng.act, eng.sh, eng.layout.Vpad
M, L, P = a["M"], a["L"], sh.P
ulog = eng.ws[("guided_uncond_logits", a["logits"].dtype)][:M * Vp].view(M, Vp)
ulse = eng.ws[("guided_uncond_lse", torch.float32)][:M]
assert a["logits"].dtype == torch.bfloat16
g1 = lambda: eng.guided_loss([1.5], ulog, ulse)
g8 = lambda: eng.guided_loss(SCALES8, ulog, ulse)
lfwd = lambda: eng.loss(batch["rating"], 3, batch_den=B)
for f in (drop, casts, g1, g8, lfwd):
    for _ in range(3):
        f()
drop_ms, drop_min = kernel_ms(drop)
cast_ms, _ = kernel_ms(casts)
g1_ms, g1_min = kernel_ms(g1)
g8_ms, g8_min = kernel_ms(g8)
lfwd_ms, lfwd_min = kernel_ms(lfwd)
ce8 = eng.guided_loss(SCALES8, ulog, ulse).tolist()
guided_bytes = 2.0 * 2.0 * B * (L - 1) * sh.V
loss_bytes = 2.0 * M * sh.V
floor_ms = 1e3 * guided_bytes / HBM_BPS

med = {name: statistics.median(v) for name, v in ms.items()}
diff = [x - y for x, y in zip(ms["drop"], ms["plain"])]
print("experience dropout at the full bf16 configuration: %d rows x %d positions, dropout on; %d alternating rounds of %d steps, "
      "milliseconds per step" % (B, T, ROUNDS, STEPS))
for name in ("plain", "drop"):
    print("%-5s  median %7.3f  mean %7.3f  min %7.3f  max %7.3f   %9.0f tokens/s (median)" % (
        name, med[name], statistics.mean(ms[name]), min(ms[name]), max(ms[name]), 1e3 * B * T / med[name]))
print("drop - plain per round: median %+7.3f  min %+7.3f  max %+7.3f  (%.2f %% of the plain step); %d of %d rows dropped in the last step" % (
    statistics.median(diff), min(diff), max(diff), 100.0 * statistics.median(diff) / med["plain"], dropped, B))
print("mmtg_experience_drop alone (%d x %d fp32 -> bf16, both channels): median %.4f ms (min %.4f); the two mmtg_cast_f32_to launches it "
      "replaces: %.4f ms" % (B, n, drop_ms, drop_min, cast_ms))
print("mmtg_guided_loss on 2 x %d x %d bf16 logits (%d loss rows): K = 1 median %.4f ms (min %.4f), K = 8 median %.4f ms (min %.4f); floor "
      "%.4f ms for %.1f MB at 8 TB/s" % (M, sh.V, B * (L - 1), g1_ms, g1_min, g8_ms, g8_min, floor_ms, guided_bytes * 1e-6))
print("mmtg_loss_fwd on one of the matrices (%d rows, %.1f MB): median %.4f ms (min %.4f); per matrix read mmtg_guided_loss takes %.2f (K = 1) "
      "and %.2f (K = 8) times that" % (M, loss_bytes * 1e-6, lfwd_ms, lfwd_min, g1_ms / 2 / lfwd_ms, g8_ms / 2 / lfwd_ms))
print("guided validation loss of the untrained model at scales", SCALES8, ":", ["%.4f" % v for v in ce8])
print(json.dumps({
    "tool": "bench_cfg", "rows": B, "positions": T, "rounds": ROUNDS, "steps_per_block": STEPS, "experience_drop": PDROP,
    "step_ms_plain": round(med["plain"], 4), "step_ms_drop": round(med["drop"], 4),
    "step_ms_diff_median": round(statistics.median(diff), 4), "step_ms_diff_min": round(min(diff), 4), "step_ms_diff_max": round(max(diff), 4),
    "step_cost_percent": round(100.0 * statistics.median(diff) / med["plain"], 3),
    "experience_drop_ms": round(drop_ms, 4), "two_casts_ms": round(cast_ms, 4),
    "guided_loss_k1_ms": round(g1_ms, 4), "guided_loss_k8_ms": round(g8_ms, 4), "loss_fwd_ms": round(lfwd_ms, 4),
    "guided_floor_bytes_ms": round(floor_ms, 5), "guided_per_matrix_over_loss_fwd_k1": round(g1_ms / 2 / lfwd_ms, 3),
    "guided_per_matrix_over_loss_fwd_k8": round(g8_ms / 2 / lfwd_ms, 3), "finite": bool(torch.isfinite(eng.master).all())}))
