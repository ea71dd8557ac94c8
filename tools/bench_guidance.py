"""Classifier-free guidance (GuidedDecoder): what the step's two extra launches cost (12-layer base model, bf16, 220 positions,
graph replay).

    python tools/bench_guidance.py [--prompts 128] [--length 220] [--reps 3]

A guided generation of N prompts runs the token step on 2 N rows, so its yardstick is the plain sampler at 2 N rows.  In one process,
alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin() apart) of a sampled
generation (temperature 1.1, top_k 10, top_p 0.7, penalty 1.5) of
  * guided:              GuidedDecoder of N prompts beside their negatives (the experience zeroed), guidance_scale 3: the step on 2 N
                         rows + mmtg_decode_guidance + the selection over N rows + mmtg_decode_mirror;
  * plain / plain_again: GreedyDecoder at 2 N rows, twice -- the distance between the two medians is the spread between equal cases
                         of this run.
guided - plain is what the two launches cost, less what the selection saves on N rows instead of 2 N.  One JSON line per measurement,
then a summary line with the medians (measuring guide: same box, alternating, medians)."""
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
    ap.add_argument("--prompts", type=int, default=128)
    ap.add_argument("--length", type=int, default=220)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import GreedyDecoder, GuidedDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance.py needs the GPU")
    S, V, N = 5, 13317, a.prompts
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    raw = synth.make_batch(2 * N, mcfg, dcfg, V, seed=7)
    batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in raw.items() if k not in ("rating", "targets")}
    prompts = {k: v[:N] for k, v in batch.items()}
    negative = {k: (torch.zeros_like(v) if k in ("img_embs", "r_embs") else v) for k, v in prompts.items()}
    guided, plain = GuidedDecoder(model, N, max_len=a.length), GreedyDecoder(model, 2 * N, max_len=a.length)
    kw = dict(temperature=1.1, repitition_penalty=1.5, top_k=10, top_p=0.7)
    cases = ("guided", "plain", "plain_again")

    def step(name):
        dec = guided if name == "guided" else plain
        gen = torch.Generator(device="cuda").manual_seed(3)
        torch.cuda.synchronize()
        if name == "guided":
            n_steps = dec.begin(prompts, negative, a.length, 3.0, generator=gen, **kw)
        else:
            n_steps = dec.begin(batch, a.length, generator=gen, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(case=name, rows=dec.B, length=a.length, steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    for name in cases[:2]:                  # warm-up: graph capture, module loading
        step(name)
    res = {name: [] for name in cases}
    for _ in range(a.reps):
        for name in cases:
            r = step(name)
            res[name].append(r["us_per_step"])
            print(json.dumps(r), flush=True)
    med = {name: statistics.median(v) for name, v in res.items()}
    print(json.dumps(dict(summary=True, prompts=N, rows=2 * N, length=a.length, reps=a.reps, median_us_per_step=med,
                          guided_minus_plain_us=med["guided"] - med["plain"],
                          spread_between_equal_cases_us=abs(med["plain_again"] - med["plain"]), describe=guided.describe())), flush=True)


if __name__ == "__main__":
    main()
