#!/usr/bin/env python3
"""The price of the per-modality guided validation loss kernel at the full configuration's logits (64 x 236 rows, V = 13317, bf16).

mmtg_guided_loss_multi on K = 2, 3, 4 random 15104 x 13317 bf16 matrices (row stride 13320) with G = 1 and G = 8 scale tuples, and
beside it, in the same process, mmtg_guided_loss -- the yardstick -- with one scale and with eight on two of the same matrices.  The
cases run as interleaved blocks (sibling, K = 2, K = 3, K = 4, at G = 1 and then at G = 8), and every round runs the whole sequence
TWICE, so that each case has two series of equal measurements: their medians' distance is the run's own spread.  A measurement is one
event pair around PER back-to-back launches.

Prints medians, minima, the bytes moved (the loss rows of the K matrices once), TB/s, the time per byte against the sibling's at one
scale, and ONE JSON line, appended to profiles/bench_mgloss.jsonl.  ROUNDS=<n> (default 10, at least 5), PER=<launches per
measurement> (default 5), ROWS=<samples> (default 64)."""
import json
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from mmtg_amd import hip

DEV = "cuda"
ROUNDS = max(5, int(os.environ.get("ROUNDS", "10")))
PER = max(1, int(os.environ.get("PER", "5")))
B, P, L, V = int(os.environ.get("ROWS", "64")), 15, 221, 13317
LDL = (V + 7) // 8 * 8
M = B * (P + L)
SCALES8 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 7.5]
TUPLES8 = [(0.0, 1.0, 1.5), (0.5, 2.0, 1.0), (1.0, 3.0, 0.5), (1.5, 1.5, 1.5), (2.0, 0.0, 2.0), (3.0, 1.0, 0.0), (5.0, 0.5, 3.0), (7.5, 7.5, 7.5)]
MARGIN = 0.10
if not torch.cuda.is_available():
    sys.exit("bench_mgloss: needs the MI355X (a timing on the host says nothing)")

gen = torch.Generator(device=DEV).manual_seed(5)
mats, lses = [], []
for k in range(hip.GUIDED_MAX_BRANCHES):
    x = (torch.randn(M, LDL, device=DEV, generator=gen) * 4.0).to(torch.bfloat16)
    mats.append(x)
    lses.append(torch.cat([torch.logsumexp(x[lo:lo + 1024, :V].float(), 1) for lo in range(0, M, 1024)]))
targets = torch.randint(0, V, (B, L), device=DEV, generator=gen)
nll = torch.empty(8 * M, device=DEV)
smp = torch.empty(8 * B, device=DEV)
ce = torch.empty(8, device=DEV)


def sibling(scales):
    return lambda: hip.guided_loss(mats[0], mats[1], LDL, V, lses[0], lses[1], None, targets, scales, B, P, L, float(B), nll, smp, ce)


def multi(K, tuples):
    tuples = [t[:K - 1] for t in tuples]
    return lambda: hip.guided_loss_multi(mats[:K], lses[:K], LDL, V, targets, tuples, B, P, L, float(B), nll, smp, ce)


CASES = [("guided_loss_s1", 2, sibling([1.5])), ("multi_k2_g1", 2, multi(2, TUPLES8[:1])), ("multi_k3_g1", 3, multi(3, TUPLES8[:1])),
         ("multi_k4_g1", 4, multi(4, TUPLES8[:1])), ("guided_loss_s8", 2, sibling(SCALES8)), ("multi_k2_g8", 2, multi(2, TUPLES8)),
         ("multi_k3_g8", 3, multi(3, TUPLES8)), ("multi_k4_g8", 4, multi(4, TUPLES8))]


def measure(launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(PER):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / PER


for _, _, f in CASES:                   # warm-up
    for _ in range(3):
        f()
torch.cuda.synchronize()
ms = {name: ([], []) for name, _, _ in CASES}
for _ in range(ROUNDS):
    for half in (0, 1):
        for name, _, f in CASES:
            ms[name][half].append(measure(f))

# the two agree at K = 2 (one distribution, two orders of operations): a word on the numbers the timings belong to
sibling([1.5, 3.0])()
a = ce[:2].clone()
multi(2, [(1.5,), (3.0,)])()
agree = float((ce[:2] - a).abs().max())

res = {}
for name, K, _ in CASES:
    both = ms[name][0] + ms[name][1]
    med = statistics.median(both)
    nbytes = 2.0 * K * B * (L - 1) * V
    res[name] = {"median_ms": med, "min_ms": min(both), "bytes": nbytes, "tb_per_s": nbytes / (med * 1e-3) * 1e-12,
                 "ns_per_mb": med * 1e6 / (nbytes * 1e-6),
                 "spread": abs(statistics.median(ms[name][0]) - statistics.median(ms[name][1])) / med}
spread = max(r["spread"] for r in res.values())
base = res["guided_loss_s1"]["ns_per_mb"]
print("mmtg_guided_loss_multi beside mmtg_guided_loss on %d x %d bf16 logits (%d loss rows), %d rounds x 2 series of %d launches" % (
    M, V, B * (L - 1), ROUNDS, PER))
for name, K, _ in CASES:
    r = res[name]
    print("%-15s median %.4f ms  min %.4f ms  %7.1f MB  %.2f TB/s  per byte %.3f x guided_loss at one scale  (two series %.2f %% apart)" % (
        name, r["median_ms"], r["min_ms"], r["bytes"] * 1e-6, r["tb_per_s"], r["ns_per_mb"] / base, 100.0 * r["spread"]))
limit = (1.0 + MARGIN) + spread
within = {name: res[name]["ns_per_mb"] / base <= limit for name in ("multi_k2_g1", "multi_k3_g1", "multi_k4_g1")}
print("G = 1 per byte against the sibling at one scale, allowed %.3f (10 %% and the largest spread, %.2f %%): %s" % (
    limit, 100.0 * spread, ", ".join("%s %.3f %s" % (n, res[n]["ns_per_mb"] / base, "inside" if ok else "OUTSIDE") for n, ok in within.items())))
print("G = 8 against the sibling at eight scales: " + ", ".join(
    "%s %.3f x" % (n, res[n]["median_ms"] / res["guided_loss_s8"]["median_ms"]) for n in ("multi_k2_g8", "multi_k3_g8", "multi_k4_g8")))
print("ce at K = 2 against mmtg_guided_loss, scales 1.5 and 3: largest difference %.3e" % agree)
line = {"tool": "bench_mgloss", "rows": M, "V": V, "ldl": LDL, "dtype": "bf16", "rounds": ROUNDS, "launches_per_measurement": PER,
        "max_spread": round(spread, 5), "margin": MARGIN, "g1_within_margin": within, "k2_ce_difference": agree}
for name, r in res.items():
    line[name] = {k: round(v, 5) if k != "bytes" else v for k, v in r.items()}
    line[name]["per_byte_over_guided_loss_s1"] = round(r["ns_per_mb"] / base, 4)
for n in ("multi_k2_g8", "multi_k3_g8", "multi_k4_g8"):
    line[n]["over_guided_loss_s8"] = round(res[n]["median_ms"] / res["guided_loss_s8"]["median_ms"], 4)
print(json.dumps(line))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "bench_mgloss.jsonl"), "a") as f:
    f.write(json.dumps(line) + "\n")
