"""Prefixed generation (GreedyDecoder.generate(..., prefix=...)): what the prefix-end check costs and what a given opening saves
(12-layer base model, bf16, 256 rows, 220 positions).

    python tools/bench_prefix.py [--rows 256] [--length 220] [--reps 3]

In one process, alternating within every rep:
  * step: us per token step of the plain step (no prefix: mmtg_decode_select) against the same step ending in
    mmtg_decode_select_fixed, with a prefix of [#START#] alone on every row -- fixed_end = P + 1, so no row is ever held and both
    decoders do the same work apart from the check (the replayed steps between two device synchronisations; begin() apart);
  * generate: whole generate() time (begin + steps) with a common prefix of k = 0, 1, 3, 5 lines (each row its own synthetic
    dataset lines, so every row has the same prefix length and the prefill covers it; k = 0 is no prefix at all).
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
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import GreedyDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix.py needs the GPU")
    S, V, SENT = 5, 13317, 22
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    raw = synth.make_batch(a.rows, mcfg, dcfg, V, seed=7)
    batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in raw.items() if k not in ("rating", "targets")}
    targets = np.asarray(raw["targets"])
    lines = (0, 1, 3, 5)
    prefixes = {k: (None if k == 0 else [targets[b, :1 + SENT * k].tolist() for b in range(a.rows)]) for k in lines}
    start_only = [[1]] * a.rows
    kw = dict(temperature=1.1, repitition_penalty=1.5)
    dec = GreedyDecoder(model, a.rows, max_len=a.length)

    def step(name):
        torch.cuda.synchronize()
        n_steps = dec.begin(batch, a.length, prefix=start_only if name == "fixed" else None, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(kind="step", select=name, rows=a.rows, length=a.length, steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    def gen(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.generate(batch, a.length, prefix=prefixes[k], **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return dict(kind="generate", lines=k, rows=a.rows, length=a.length, token_steps=a.length + model.engine().sh.P - dec.first_pos,
                    first_pos=dec.first_pos, generate_ms=1e3 * (t1 - t0))

    for name in ("plain", "fixed"):          # warm-up: graph capture, module loading
        step(name)
    for k in lines:
        gen(k)
    res = {"plain": [], "fixed": []}
    gres = {k: [] for k in lines}
    for _ in range(a.reps):
        for name in ("plain", "fixed"):
            r = step(name)
            res[name].append(r["us_per_step"])
            print(json.dumps(r), flush=True)
        for k in lines:
            r = gen(k)
            gres[k].append(r["generate_ms"])
            print(json.dumps(r), flush=True)
    med = {name: statistics.median(v) for name, v in res.items()}
    gmed = {str(k): statistics.median(v) for k, v in gres.items()}
    print(json.dumps(dict(summary=True, rows=a.rows, length=a.length, reps=a.reps, median_us_per_step=med,
                          fixed_over_plain_step=med["fixed"] / med["plain"], median_generate_ms_by_lines=gmed,
                          describe=dec.describe())), flush=True)


if __name__ == "__main__":
    main()
