"""Line-length bounds and line-end sets (GreedyDecoder / BeamDecoder .generate(..., line_lengths=, line_end_ids=)): what the rule
costs in the step's last launch (12-layer base model, bf16, 256 rows, 220 positions).

    python tools/bench_lines.py [--rows 256] [--length 220] [--reps 3] [--ngram 4] [--beams 4] [--lo 3] [--hi 18] [--set-size 700]
                                [--kinds greedy,sample,beam]

In one process, alternating within every rep, us per token step (the replayed steps between two device synchronisations; begin()
apart) of the step without line constraints -- the plain selection entry for n = 0, the *_ngram entry for n = --ngram: the launches
and kernels of the parent commit, which this change leaves instruction for instruction as they were -- against the same step
ending in the *_lines entry with bounds (--lo, --hi) on every line and an end set of --set-size ids on every second line, for
  * greedy: mmtg_decode_select / _ngram against mmtg_decode_select_lines;
  * sample (temperature 1.1, top-k 10, top-p 0.7, penalty 1.5, the same uniforms): mmtg_decode_sample / _ngram against
    mmtg_decode_sample_lines;
  * beam (rows / beams prompts x beams): mmtg_decode_beam_candidates / _ngram against mmtg_decode_beam_candidates_lines.
One JSON line per measurement, then a summary line: medians, the lines / base ratio, the spread (min .. max) of the base legs and
whether the lines median lies inside it (measuring guide: same box, alternating, medians)."""
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
    ap.add_argument("--lo", type=int, default=3)
    ap.add_argument("--hi", type=int, default=18)
    ap.add_argument("--set-size", type=int, default=700)
    ap.add_argument("--kinds", default="greedy,sample,beam", help="which decoders to time (a profiler run wants one)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import BeamDecoder, GreedyDecoder, check_lines
    if not torch.cuda.is_available():
        raise SystemExit("bench_lines.py needs the GPU")
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
    ends = frozenset(int(v) for v in np.random.RandomState(1).choice(np.arange(200, V), size=a.set_size, replace=False))
    spec = dict(line_lengths=(a.lo, a.hi), line_end_ids=[ends if l % 2 else None for l in range(n_lines)])
    tables = {rows: check_lines(spec["line_lengths"], spec["line_end_ids"], rows, a.length, sent, V) for rows in (a.rows, n_prompts)}
    kw = dict(temperature=1.1, repitition_penalty=1.5)
    settings = {"greedy": dict(), "sample": dict(top_k=10, top_p=0.7)}

    def step(kind, n, lines):
        d = bdec if kind == "beam" else dec
        extra = {} if kind == "beam" else dict(settings[kind], generator=torch.Generator(device="cuda").manual_seed(3))
        torch.cuda.synchronize()
        n_steps = d.begin(pbatch if kind == "beam" else batch, a.length, no_repeat_ngram_size=n,
                          line_lengths=tables[n_prompts if kind == "beam" else a.rows] if lines else None, **kw, **extra)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(d.first_pos, n_steps):
            d.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - d.first_pos
        return dict(kind=kind, ngram=n, lines=bool(lines), rows=a.rows, length=a.length, steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    kinds = tuple(a.kinds.split(","))
    ngrams = (0, a.ngram) if a.ngram else (0,)
    legs = [(k, n, ln) for k in kinds for n in ngrams for ln in (False, True)]
    for leg in legs:                        # warm-up: graph capture, module loading
        step(*leg)
    res = {leg: [] for leg in legs}
    for _ in range(a.reps):
        for leg in legs:
            r = step(*leg)
            res[leg].append(r["us_per_step"])
            print(json.dumps(r), flush=True)
    name = lambda k, n, ln: "%s_n%d_%s" % (k, n, "lines" if ln else "base")      # noqa: E731
    med = {name(*leg): statistics.median(v) for leg, v in res.items()}
    spread = {name(k, n, False): [min(res[(k, n, False)]), max(res[(k, n, False)])] for k in kinds for n in ngrams}
    ratio = {"%s_n%d" % (k, n): med[name(k, n, True)] / med[name(k, n, False)] for k in kinds for n in ngrams}
    inside = {"%s_n%d" % (k, n): spread[name(k, n, False)][0] <= med[name(k, n, True)] <= spread[name(k, n, False)][1]
              for k in kinds for n in ngrams}
    print(json.dumps(dict(summary=True, rows=a.rows, length=a.length, reps=a.reps, ngram=a.ngram, beams=a.beams, bounds=[a.lo, a.hi],
                          set_size=a.set_size, median_us_per_step=med, base_spread_us=spread, lines_over_base_step=ratio,
                          lines_median_inside_base_spread=inside, describe=dec.describe())), flush=True)


if __name__ == "__main__":
    main()
