"""Keyword-constrained beam search (BeamDecoder.generate(..., keywords=)): what the keyword candidates and merge cost in the token
step (12-layer base model, bf16, 64 prompts x 4 beams, 220 positions).

    python tools/bench_keywords.py [--prompts 64] [--beams 4] [--length 220] [--reps 3] [--legs a,b,c] [--out FILE]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of three legs:
  a  keywords=None: mmtg_decode_beam_candidates / mmtg_decode_beam_merge, the launches and graphs of a search without the argument;
  b  K = 2 keywords (two and one ids long): mmtg_decode_beam_candidates_kw / mmtg_decode_beam_merge_kw on every step with the head;
  c  K = 8 keywords (lengths 1 .. 4): with four beams W = 12 candidates per parent.
Leg a runs kernels this change leaves instruction for instruction as they were.  One JSON line per measurement, then a summary
line: medians, b - a and c - a in us and as a fraction of the a step, the spread (min .. max) of the a legs, and how many keywords the
first hypotheses of legs b and c hold.  There is no gate.  --out also appends the lines to a file; the committed record is
profiles/r16_keywords_bench.jsonl."""
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
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.constraints import keywords_met
    from mmtg_amd.decode import BeamDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_keywords.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    raw = synth.make_batch(a.prompts, mcfg, dcfg, V, seed=7)
    batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in raw.items() if k not in ("rating", "targets")}
    dec = BeamDecoder(model, a.prompts, a.beams, max_len=a.length)
    eight = [tuple(1000 + 10 * i + k for k in range(1 + i % 4)) for i in range(8)]             # lengths 1, 2, 3, 4, 1, 2, 3, 4
    specs = {"a": None, "b": [(1000, 1001), (2000,)], "c": eight}
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def step(leg):
        kw = specs[leg]
        torch.cuda.synchronize()
        n_steps = dec.begin(batch, a.length, temperature=1.1, repitition_penalty=1.5, **({} if kw is None else {"keywords": kw}))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - dec.first_pos
        rec = dict(leg=leg, keywords=0 if kw is None else len(kw), prompts=a.prompts, beams=a.beams, length=a.length, steps=steps,
                   us_per_step=1e6 * (t2 - t1) / steps)
        if kw is not None:      # (after the timing) how many keywords each prompt's best-endowed beam holds, on average
            ids = dec.seq[:, dec.eng.sh.P:dec.eng.sh.P + 1 + a.length].view(a.prompts, a.beams, -1).cpu().tolist()
            rec["mean_best_met"] = float(np.mean([max(keywords_met(r, kw) for r in p) for p in ids]))
        return rec

    names = tuple(a.legs.split(","))
    for leg in names:                       # warm-up: graph capture, module loading
        step(leg)
    res = {leg: [] for leg in names}
    met = {}
    for _ in range(a.reps):
        for leg in names:
            r = step(leg)
            res[leg].append(r["us_per_step"])
            met[leg] = r.get("mean_best_met")
            emit(r)
    med = {leg: statistics.median(v) for leg, v in res.items()}
    out = dict(summary=True, prompts=a.prompts, beams=a.beams, length=a.length, reps=a.reps, median_us_per_step=med,
               mean_best_met={k: v for k, v in met.items() if v is not None}, describe=dec.describe())
    if "a" in names:
        lo, hi = min(res["a"]), max(res["a"])
        out["a_spread_us"] = [lo, hi]
        for leg in names:
            if leg != "a":
                out[leg + "_minus_a_us"] = med[leg] - med["a"]
                out[leg + "_minus_a_over_a_step"] = (med[leg] - med["a"]) / med["a"]
    emit(out)


if __name__ == "__main__":
    main()
