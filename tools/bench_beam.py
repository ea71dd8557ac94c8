"""Beam-search token step against the greedy token step at the same row count (12-layer base model, bf16, full length).

    python tools/bench_beam.py [--prompts 64] [--beams 4] [--length 220] [--reps 5]

In one process it alternates BeamDecoder (prompts x beams rows) and GreedyDecoder (the same row count), both graph-replayed,
and reports per decoder: us per token step (the replayed steps of a generation between two device synchronisations: the
begin() work -- weight copies, folds, encoder, prompt prefill -- is timed apart), the whole generate() time, and generated
tokens/s (rows x length / generate time).  One JSON line per decoder and rep, then a summary line with the medians.
For the kernel split, run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_beam.py --reps 1`."""
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import BeamDecoder, GreedyDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    rows = a.prompts * a.beams

    def batch(n, seed):
        b = synth.make_batch(n, mcfg, dcfg, V, seed=seed)
        return {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in b.items() if k not in ("rating", "targets")}

    decs = {"beam": (BeamDecoder(model, a.prompts, a.beams, max_len=a.length), batch(a.prompts, 7)),
            "greedy": (GreedyDecoder(model, rows, max_len=a.length), batch(rows, 7))}
    kw = dict(temperature=1.1, repitition_penalty=1.5)

    def run(name):
        dec, b = decs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_steps = dec.begin(b, a.length, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out = dec.generate(b, a.length, **kw)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(decoder=name, rows=rows, length=a.length, steps=steps, begin_ms=1e3 * (t1 - t0),
                    us_per_step=1e6 * (t2 - t1) / steps, generate_ms=1e3 * (t3 - t2), tokens_per_s=rows * a.length / (t3 - t2),
                    describe=dec.describe()), out

    for name in decs:            # warm-up: graph capture, module loading
        run(name)
    res = {name: [] for name in decs}
    for _ in range(a.reps):
        for name in decs:
            r, _ = run(name)
            res[name].append(r)
            print(json.dumps(r), flush=True)
    med = {name: {k: statistics.median(x[k] for x in rs) for k in ("us_per_step", "generate_ms", "tokens_per_s", "begin_ms")}
           for name, rs in res.items()}
    print(json.dumps(dict(summary=True, prompts=a.prompts, beams=a.beams, rows=rows, length=a.length, reps=a.reps, median=med,
                          beam_over_greedy_step=med["beam"]["us_per_step"] / med["greedy"]["us_per_step"])), flush=True)


if __name__ == "__main__":
    main()
