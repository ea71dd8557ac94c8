"""Diverse beam search (BeamDecoder.generate(..., num_beam_groups=, diversity_penalty=)): what the grouped merge costs in the token
step (12-layer base model, bf16, 64 prompts x 4 beams, 220 positions).

    python tools/bench_groups.py [--prompts 64] [--beams 4] [--length 220] [--reps 3] [--penalty 0.5] [--legs a,b,c]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of three legs:
  a  one group: mmtg_decode_beam_merge, the launches and graphs of a search without the arguments;
  b  two groups at --penalty: mmtg_decode_beam_merge_groups on every step that calls the head;
  c  --beams groups (one beam each) at --penalty.
Leg a runs kernels this change leaves instruction for instruction as they were.  One JSON line per measurement, then a summary
line: medians, b - a and c - a in us and as a fraction of the a step, the spread (min .. max) of the a legs, and whether b and c lie
within that spread plus 1 % of the a step (measuring guide: same box, alternating, medians).  The committed record is
profiles/r15_groups_bench.jsonl."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=64)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--length", type=int, default=220)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--penalty", type=float, default=0.5)
    ap.add_argument("--legs", default="a,b,c")
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import BeamDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_groups.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    raw = synth.make_batch(a.prompts, mcfg, dcfg, V, seed=7)
    batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in raw.items() if k not in ("rating", "targets")}
    dec = BeamDecoder(model, a.prompts, a.beams, max_len=a.length)
    specs = {"a": dict(), "b": dict(num_beam_groups=2, diversity_penalty=a.penalty),
             "c": dict(num_beam_groups=a.beams, diversity_penalty=a.penalty)}

    def step(leg):
        torch.cuda.synchronize()
        n_steps = dec.begin(batch, a.length, temperature=1.1, repitition_penalty=1.5, **specs[leg])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(leg=leg, groups=dec.rules.groups, penalty=dec.rules.diversity_penalty, prompts=a.prompts, beams=a.beams, length=a.length,
                    steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    names = tuple(a.legs.split(","))
    for leg in names:                       # warm-up: graph capture, module loading
        step(leg)
    res = {leg: [] for leg in names}
    for _ in range(a.reps):
        for leg in names:
            r = step(leg)
            res[leg].append(r["us_per_step"])
            print(json.dumps(r), flush=True)
    med = {leg: statistics.median(v) for leg, v in res.items()}
    out = dict(summary=True, prompts=a.prompts, beams=a.beams, length=a.length, reps=a.reps, penalty=a.penalty, median_us_per_step=med,
               describe=dec.describe())
    if "a" in names:
        lo, hi = min(res["a"]), max(res["a"])
        out["a_spread_us"] = [lo, hi]
        for leg in names:
            if leg != "a":
                out[leg + "_minus_a_us"] = med[leg] - med["a"]
                out[leg + "_minus_a_over_a_step"] = (med[leg] - med["a"]) / med["a"]
                out[leg + "_within_a_spread_plus_1pct"] = med[leg] - med["a"] <= (hi - lo) + 0.01 * med["a"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
