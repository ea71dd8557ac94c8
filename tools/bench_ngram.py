"""n-gram blocking (GreedyDecoder / BeamDecoder .generate(..., no_repeat_ngram_size=n)): what the ban scan in the step's last launch
costs (12-layer base model, bf16, 256 rows, 220 positions).

    python tools/bench_ngram.py [--rows 256] [--length 220] [--reps 3] [--ngram 4] [--beams 4]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of the plain step against the same step ending in the *_ngram selection entry, for
  * greedy: mmtg_decode_select against mmtg_decode_select_ngram;
  * sample (temperature 1.1, top-k 10, top-p 0.7, penalty 1.5, the same uniforms): mmtg_decode_sample against
    mmtg_decode_sample_ngram;
  * beam (rows / beams prompts x beams): mmtg_decode_beam_candidates against mmtg_decode_beam_candidates_ngram.
One JSON line per measurement, then a summary line with the medians (measuring guide: same box, alternating, medians)."""
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
    ap.add_argument("--ngram", type=int, default=4)
    ap.add_argument("--beams", type=int, default=4)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import BeamDecoder, GreedyDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_ngram.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    raw = synth.make_batch(a.rows, mcfg, dcfg, V, seed=7)
    batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in raw.items() if k not in ("rating", "targets")}
    n_prompts = a.rows // a.beams
    pbatch = {k: v[:n_prompts] for k, v in batch.items()}
    dec = GreedyDecoder(model, a.rows, max_len=a.length)
    bdec = BeamDecoder(model, n_prompts, a.beams, max_len=a.length)
    kw = dict(temperature=1.1, repitition_penalty=1.5)
    settings = {"greedy": dict(), "sample": dict(top_k=10, top_p=0.7)}

    def step(kind, n):
        d = bdec if kind == "beam" else dec
        extra = {} if kind == "beam" else dict(settings[kind], generator=torch.Generator(device="cuda").manual_seed(3))
        torch.cuda.synchronize()
        n_steps = d.begin(pbatch if kind == "beam" else batch, a.length, no_repeat_ngram_size=n, **kw, **extra)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(d.first_pos, n_steps):
            d.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - d.first_pos
        return dict(kind=kind, ngram=n, rows=a.rows, length=a.length, steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    kinds = ("greedy", "sample", "beam")
    for kind in kinds:                      # warm-up: graph capture, module loading
        for n in (0, a.ngram):
            step(kind, n)
    res = {(k, n): [] for k in kinds for n in (0, a.ngram)}
    for _ in range(a.reps):
        for kind in kinds:
            for n in (0, a.ngram):
                r = step(kind, n)
                res[(kind, n)].append(r["us_per_step"])
                print(json.dumps(r), flush=True)
    med = {"%s_n%d" % k: statistics.median(v) for k, v in res.items()}
    ratio = {k: med["%s_n%d" % (k, a.ngram)] / med["%s_n0" % k] for k in kinds}
    print(json.dumps(dict(summary=True, rows=a.rows, length=a.length, reps=a.reps, ngram=a.ngram, beams=a.beams,
                          median_us_per_step=med, ngram_over_plain_step=ratio, describe=dec.describe())), flush=True)


if __name__ == "__main__":
    main()
