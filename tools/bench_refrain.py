"""Refrain schemes (GreedyDecoder / BeamDecoder .generate(..., refrain_scheme=)): what the form costs in the step's last launch and
what skipping the head on copy columns saves (12-layer base model, bf16, 256 rows, 220 positions).

    python tools/bench_refrain.py [--rows 256] [--length 220] [--reps 3] [--beams 4] [--lo 3] [--hi 18] [--classes 12]
                                  [--class-size 500] [--scheme AB.AB.AB.A] [--kinds greedy,sample,beam] [--legs a,b,c,d]
                                  [--out profiles/r17_refrain_bench.jsonl]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of four legs:
  a  no constraints: the plain selection entry -- the launches of a generation without the argument;
  b  the *_rhyme entry, an acrostic: one given id opens every line (an open template), bounds (--lo, --hi) on every line, under a
     rhyme scheme of dots over --classes classes of --class-size ids (tools/bench_rhyme.py's leg b through the rhyme form);
  c  the *_refrain entry over b's tables with no line a copy ("ABCDEFGHIJ"): the form's overhead;
  d  --scheme alone (no other constraint): five of ten lines are copies.  Greedy and sampling skip the head on their columns
     (every row copies); the beams do not (their merge knows nothing of copies), so for them d is the form on the bare tables;
for greedy (mmtg_decode_select*), sample (temperature 1.1, top-k 10, top-p 0.7, penalty 1.5, the same uniforms: mmtg_decode_sample*)
and beam (rows / beams prompts x beams: mmtg_decode_beam_candidates*).  Legs a and b run kernels this change leaves instruction for
instruction as they were.  One JSON line per measurement (with the number of steps that called the head), then a summary line:
medians, c - b and d - a in us and as a fraction of the a step, the spread (min .. max) of the a legs, whether c lies within that
spread of b, and for d the steps that skipped the head.  The lines are printed and written to --out (measuring guide: same box,
alternating, medians).  Needs nothing but the tree: synthetic weights and inputs."""
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
    ap.add_argument("--scheme", default="AB.AB.AB.A")
    ap.add_argument("--kinds", default="greedy,sample,beam", help="which decoders to time (a profiler run wants one)")
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_refrain_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.constraints import _check_constraints
    from mmtg_amd.decode import BeamDecoder, GreedyDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_refrain.py needs the GPU")
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
    sh = dec.eng.sh
    sent = sh.msl + 2
    n_lines = (a.length - 1) // sent + 1
    rng = np.random.RandomState(1)
    pool = rng.permutation(np.arange(200, V))
    classes = [frozenset(int(v) for v in pool[i * a.class_size:(i + 1) * a.class_size]) for i in range(a.classes)]
    heads = [int(v) for v in pool[a.classes * a.class_size:a.classes * a.class_size + n_lines]]
    acro = dict(line_lengths=(a.lo, a.hi), templates=[(v, Ellipsis) for v in heads], rhyme_scheme="." * n_lines, rhyme_classes=classes)
    letters = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
    specs = {"a": None, "b": acro, "c": dict(acro, refrain_scheme=letters[:n_lines]), "d": dict(refrain_scheme=a.scheme[:n_lines])}

    def tables(sp, rows):
        if sp is None:
            return None
        return _check_constraints(None, 0, sp.get("line_lengths"), None, rows, a.length, sh, "%d rows" % rows, sp.get("templates"),
                                  sp.get("rhyme_scheme"), sp.get("rhyme_classes"), False, sp.get("refrain_scheme")).lines
    tabs = {(leg, rows): tables(sp, rows) for leg, sp in specs.items() for rows in (a.rows, n_prompts)}
    kw = dict(temperature=1.1, repitition_penalty=1.5)
    settings = {"greedy": dict(), "sample": dict(top_k=10, top_p=0.7)}

    def step(kind, leg):
        d = bdec if kind == "beam" else dec
        extra = {} if kind == "beam" else dict(settings[kind], generator=torch.Generator(device="cuda").manual_seed(3))
        torch.cuda.synchronize()
        n_steps = d.begin(pbatch if kind == "beam" else batch, a.length, line_lengths=tabs[(leg, n_prompts if kind == "beam" else a.rows)],
                          **kw, **extra)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        heads_run = 0
        for pos in range(d.first_pos, n_steps):
            heads_run += bool(d.step_at(pos))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - d.first_pos
        return dict(kind=kind, leg=leg, rows=a.rows, length=a.length, steps=steps, head_steps=heads_run, skipped_steps=d.skipped_steps,
                    us_per_step=1e6 * (t2 - t1) / steps)

    kinds = tuple(a.kinds.split(","))
    names = tuple(a.legs.split(","))
    legs = [(k, leg) for k in kinds for leg in names]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    for leg in legs:                        # warm-up: graph capture, module loading
        step(*leg)
    res = {leg: [] for leg in legs}
    skipped = {}
    for _ in range(a.reps):
        for leg in legs:
            r = step(*leg)
            res[leg].append(r["us_per_step"])
            skipped[leg] = r["skipped_steps"]
            emit(r)
    med = {"%s_%s" % leg: statistics.median(v) for leg, v in res.items()}
    out = dict(summary=True, rows=a.rows, length=a.length, reps=a.reps, beams=a.beams, bounds=[a.lo, a.hi], scheme=a.scheme[:n_lines],
               classes=a.classes, class_size=a.class_size, median_us_per_step=med, describe=dec.describe())
    if "a" in names:
        out["a_spread_us"] = {k: [min(res[(k, "a")]), max(res[(k, "a")])] for k in kinds}
        spread = {k: max(res[(k, "a")]) - min(res[(k, "a")]) for k in kinds}
        if "b" in names:
            out["b_minus_a_over_a_step"] = {k: (med[k + "_b"] - med[k + "_a"]) / med[k + "_a"] for k in kinds}
        if "b" in names and "c" in names:
            out["c_minus_b_us"] = {k: med[k + "_c"] - med[k + "_b"] for k in kinds}
            out["c_minus_a_over_a_step"] = {k: (med[k + "_c"] - med[k + "_a"]) / med[k + "_a"] for k in kinds}
            out["c_within_a_spread_of_b"] = {k: med[k + "_c"] - med[k + "_b"] <= spread[k] for k in kinds}
        if "d" in names:
            out["d_minus_a_us"] = {k: med[k + "_d"] - med[k + "_a"] for k in kinds}
            out["d_minus_a_over_a_step"] = {k: (med[k + "_d"] - med[k + "_a"]) / med[k + "_a"] for k in kinds}
            out["d_skipped_steps"] = {k: skipped[(k, "d")] for k in kinds}
    emit(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
