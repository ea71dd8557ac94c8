"""Token log-probabilities (GreedyDecoder .generate(..., return_logprobs=True)): what the extra graph node behind the selection,
mmtg_decode_logprob, costs per token step (12-layer base model, bf16, 256 rows, 220 positions).

    python tools/bench_logprob.py [--rows 256] [--length 220] [--reps 3] [--out profiles/r14_logprob_bench.jsonl]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of leg a, the step without the argument (the launches of a generation without it), against leg b, the same step with
return_logprobs, for
  * greedy: mmtg_decode_select, then mmtg_decode_logprob;
  * sample (temperature 1.1, top-k 10, top-p 0.7, penalty 1.5, the same uniforms): mmtg_decode_sample, then mmtg_decode_logprob.
One JSON line per measurement, then a summary line with the medians, the spread of the a legs (max - min over the reps: what a
difference has to exceed to mean anything) and b - a (measuring guide: same box, alternating, medians).  --out appends the lines
to a file as well."""
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
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--length", type=int, default=220)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import GreedyDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_logprob.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    raw = synth.make_batch(a.rows, mcfg, dcfg, V, seed=7)
    batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in raw.items() if k not in ("rating", "targets")}
    dec = GreedyDecoder(model, a.rows, max_len=a.length)
    kw = dict(temperature=1.1, repitition_penalty=1.5)
    settings = {"greedy": dict(), "sample": dict(top_k=10, top_p=0.7)}
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def step(kind, lp):
        extra = dict(settings[kind], generator=torch.Generator(device="cuda").manual_seed(3))
        torch.cuda.synchronize()
        n_steps = dec.begin(batch, a.length, **kw, **extra, **({"return_logprobs": True} if lp else {}))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        heads = 0
        for pos in range(dec.first_pos, n_steps):
            heads += bool(dec.step_at(pos))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(kind=kind, leg="b" if lp else "a", return_logprobs=bool(lp), rows=a.rows, length=a.length, steps=steps,
                    head_steps=heads, us_per_step=1e6 * (t2 - t1) / steps)

    kinds = ("greedy", "sample")
    for kind in kinds:                      # warm-up: graph capture, module loading
        for lp in (False, True):
            step(kind, lp)
    res = {(k, lp): [] for k in kinds for lp in (False, True)}
    heads = steps = 0
    for _ in range(a.reps):
        for kind in kinds:
            for lp in (False, True):
                r = step(kind, lp)
                res[(kind, lp)].append(r["us_per_step"])
                heads, steps = r["head_steps"], r["steps"]
                emit(r)
    med = {"%s_%s" % (k, "b" if lp else "a"): statistics.median(v) for (k, lp), v in res.items()}
    spread = {k: max(res[(k, False)]) - min(res[(k, False)]) for k in kinds}
    delta = {k: med[k + "_b"] - med[k + "_a"] for k in kinds}
    emit(dict(summary=True, rows=a.rows, length=a.length, reps=a.reps, steps=steps, head_steps=heads, median_us_per_step=med,
              a_spread_us=spread, b_minus_a_us_per_step=delta,
              b_minus_a_us_per_head_step={k: delta[k] * steps / max(heads, 1) for k in kinds}, describe=dec.describe()))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
