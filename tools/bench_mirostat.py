"""Mirostat sampling (GreedyDecoder.generate(..., mirostat_tau= / mirostat_eta=)): what the stage and its per-row state cost in the
step's last launch (12-layer base model, bf16, 256 rows, 220 positions, graph replay).

    python tools/bench_mirostat.py [--rows 256] [--length 220] [--reps 3]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of a sampled generation (temperature 1.1, top_k 0, top_p 0, penalty 1.5, the same uniforms) that ends in
  * off / off_again: mmtg_decode_sample (the rules off: the step as it was, twice -- the distance between the two medians is the
                     spread between equal cases of this run);
  * mirostat:        mmtg_decode_sample_mirostat at mirostat_tau = 2, mirostat_eta = 0.1;
  * typical_p:       mmtg_decode_sample_warp at typical_p = 0.9, for scale;
  * both:            mmtg_decode_sample_mirostat behind typical_p = 0.9.
One JSON line per measurement, then a summary line with the medians and the extra us per step of every case over `off`
(measuring guide: same box, alternating, medians)."""
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
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import GreedyDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_mirostat.py needs the GPU")
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
    opened = dict(top_k=0, top_p=0.0)
    cases = {"off": opened, "mirostat": dict(opened, mirostat_tau=2.0, mirostat_eta=0.1), "typical_p": dict(opened, typical_p=0.9),
             "both": dict(opened, typical_p=0.9, mirostat_tau=2.0, mirostat_eta=0.1), "off_again": opened}
    base = {name: "off" for name in cases}

    def step(name):
        torch.cuda.synchronize()
        n_steps = dec.begin(batch, a.length, generator=torch.Generator(device="cuda").manual_seed(3), **kw, **cases[name])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(case=name, rows=a.rows, length=a.length, steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    for name in cases:                      # warm-up: graph capture, module loading
        step(name)
    res = {name: [] for name in cases}
    for _ in range(a.reps):
        for name in cases:
            r = step(name)
            res[name].append(r["us_per_step"])
            print(json.dumps(r), flush=True)
    med = {name: statistics.median(v) for name, v in res.items()}
    extra = {name: med[name] - med[base[name]] for name in cases if name != base[name]}
    # (two columns in 22 are forced [#START#] / [#EOS#] and call no head: the cost falls on the other twenty)
    print(json.dumps(dict(summary=True, rows=a.rows, length=a.length, reps=a.reps, median_us_per_step=med, extra_us_per_step=extra,
                          spread_between_equal_cases_us=abs(med["off_again"] - med["off"]),
                          final_mu_mean=float(dec.mirostat_mu.mean()) if dec.mirostat_mu is not None else None,
                          describe=dec.describe())), flush=True)


if __name__ == "__main__":
    main()
