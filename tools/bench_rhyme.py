"""Rhyme schemes (GreedyDecoder / BeamDecoder .generate(..., rhyme_scheme=)): what the rule costs in the step's last launch (12-layer
base model, bf16, 256 rows, 220 positions).

    python tools/bench_rhyme.py [--rows 256] [--length 220] [--reps 3] [--beams 4] [--lo 3] [--hi 18] [--classes 12]
                                [--class-size 500] [--scheme AABBAABBAA] [--kinds greedy,sample,beam] [--legs a,b,c,d]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of four legs:
  a  no constraints: the plain selection entry;
  b  the *_tmpl entry, an acrostic: one given id opens every line (an open template), bounds (--lo, --hi) on every line;
  c  the *_rhyme entry: b's templates and bounds under --scheme over --classes classes of --class-size ids;
  d  c with rhyme_distinct;
for greedy (mmtg_decode_select*), sample (temperature 1.1, top-k 10, top-p 0.7, penalty 1.5, the same uniforms: mmtg_decode_sample*)
and beam (rows / beams prompts x beams: mmtg_decode_beam_candidates*).  Legs a and b run kernels this change leaves instruction for
instruction as they were.  One JSON line per measurement, then a summary line: medians, c / b and d / b, c - a and d - a as a
fraction of the a step, the spread (min .. max) of the a legs, and whether c and d lie within that spread of b (measuring guide: same
box, alternating, medians)."""
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
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--lo", type=int, default=3)
    ap.add_argument("--hi", type=int, default=18)
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--class-size", type=int, default=500)
    ap.add_argument("--scheme", default="AABBAABBAA")
    ap.add_argument("--kinds", default="greedy,sample,beam", help="which decoders to time (a profiler run wants one)")
    ap.add_argument("--legs", default="a,b,c,d")
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_lines
    if not torch.cuda.is_available():
        raise SystemExit("bench_rhyme.py needs the GPU")
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
    sent = dec.eng.sh.msl + 2
    n_lines = (a.length - 1) // sent + 1
    rng = np.random.RandomState(1)
    pool = rng.permutation(np.arange(200, V))
    classes = [frozenset(int(v) for v in pool[i * a.class_size:(i + 1) * a.class_size]) for i in range(a.classes)]
    heads = [int(v) for v in pool[a.classes * a.class_size:a.classes * a.class_size + n_lines]]
    acro = dict(line_lengths=(a.lo, a.hi), templates=[(v, Ellipsis) for v in heads])
    rhyme = dict(acro, rhyme_scheme=a.scheme[:n_lines], rhyme_classes=classes)
    specs = {"a": None, "b": acro, "c": rhyme, "d": dict(rhyme, rhyme_distinct=True)}
    tables = {(leg, rows): None if sp is None else check_lines(sp["line_lengths"], None, rows, a.length, sent, V,
                                                               **{k: v for k, v in sp.items() if k != "line_lengths"})
              for leg, sp in specs.items() for rows in (a.rows, n_prompts)}
    kw = dict(temperature=1.1, repitition_penalty=1.5)
    settings = {"greedy": dict(), "sample": dict(top_k=10, top_p=0.7)}

    def step(kind, leg):
        d = bdec if kind == "beam" else dec
        extra = {} if kind == "beam" else dict(settings[kind], generator=torch.Generator(device="cuda").manual_seed(3))
        torch.cuda.synchronize()
        n_steps = d.begin(pbatch if kind == "beam" else batch, a.length, line_lengths=tables[(leg, n_prompts if kind == "beam" else a.rows)],
                          **kw, **extra)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(d.first_pos, n_steps):
            d.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - d.first_pos
        return dict(kind=kind, leg=leg, rows=a.rows, length=a.length, steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    kinds = tuple(a.kinds.split(","))
    names = tuple(a.legs.split(","))
    legs = [(k, leg) for k in kinds for leg in names]
    for leg in legs:                        # warm-up: graph capture, module loading
        step(*leg)
    res = {leg: [] for leg in legs}
    for _ in range(a.reps):
        for leg in legs:
            r = step(*leg)
            res[leg].append(r["us_per_step"])
            print(json.dumps(r), flush=True)
    med = {"%s_%s" % leg: statistics.median(v) for leg, v in res.items()}
    out = dict(summary=True, rows=a.rows, length=a.length, reps=a.reps, beams=a.beams, bounds=[a.lo, a.hi], scheme=a.scheme[:n_lines],
               classes=a.classes, class_size=a.class_size, median_us_per_step=med, describe=dec.describe())
    if "a" in names:
        out["a_spread_us"] = {k: [min(res[(k, "a")]), max(res[(k, "a")])] for k in kinds}
    if "b" in names:
        for leg in ("c", "d"):
            if leg in names:
                out[leg + "_over_b_step"] = {k: med["%s_%s" % (k, leg)] / med[k + "_b"] for k in kinds}
                out[leg + "_minus_b_us"] = {k: med["%s_%s" % (k, leg)] - med[k + "_b"] for k in kinds}
                if "a" in names:
                    out[leg + "_minus_a_over_a_step"] = {k: (med["%s_%s" % (k, leg)] - med[k + "_a"]) / med[k + "_a"] for k in kinds}
                    out["b_minus_a_over_a_step"] = {k: (med[k + "_b"] - med[k + "_a"]) / med[k + "_a"] for k in kinds}
                    out[leg + "_within_a_spread_of_b"] = {
                        k: abs(med["%s_%s" % (k, leg)] - med[k + "_b"]) <= max(res[(k, "a")]) - min(res[(k, "a")]) for k in kinds}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
