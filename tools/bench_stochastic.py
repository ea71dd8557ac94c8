"""Stochastic-beam-search token step against the beam-search token step on the same prompts (12-layer base model, bf16, full length),
and the two new launches on their own beside the beam launches they stand in for.

    python tools/bench_stochastic.py [--prompts 64] [--samples 4] [--length 220] [--reps 3]

In one process it alternates StochasticBeamDecoder (prompts x samples rows) and BeamDecoder (prompts, as many beams: the same rows,
the same prompts), both graph-replayed, and reports per decoder what tools/bench_beam.py reports: us per token step (the replayed
steps of a generation between two device synchronisations; begin() is timed apart), the whole generate() time, tokens/s.  One JSON
line per decoder and rep, then a summary line with the medians.  The beam decoder's launches are the parent's, unchanged, so the
beam leg is the baseline of the same run.
Then mmtg_decode_gumbel_candidates / mmtg_decode_gumbel_merge and mmtg_decode_beam_candidates / mmtg_decode_beam_merge alone, on the
stochastic decoder's own buffers as the generation left them, at a free lyric column: 50 launches captured in one graph, replayed,
device events around the replays; one JSON line with us per launch of each.
For the kernel split, run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_stochastic.py --reps 1`."""
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
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--length", type=int, default=220)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, hip, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import BeamDecoder, StochasticBeamDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_stochastic.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    nb, rows = a.samples, a.prompts * a.samples
    b = synth.make_batch(a.prompts, mcfg, dcfg, V, seed=7)
    batch = {key: torch.from_numpy(np.asarray(v)).cuda() for key, v in b.items() if key not in ("rating", "targets")}
    decs = {"stochastic": (StochasticBeamDecoder(model, a.prompts, nb, max_len=a.length), dict(seed=0)),
            "beam": (BeamDecoder(model, a.prompts, nb, max_len=a.length), {})}
    kw = dict(temperature=1.1, repitition_penalty=1.5)

    def run(name):
        dec, extra = decs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_steps = dec.begin(batch, a.length, **kw, **extra)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dec.generate(batch, a.length, **kw, **extra)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(decoder=name, rows=rows, length=a.length, steps=steps, begin_ms=1e3 * (t1 - t0),
                    us_per_step=1e6 * (t2 - t1) / steps, generate_ms=1e3 * (t3 - t2), tokens_per_s=rows * a.length / (t3 - t2),
                    describe=dec.describe())

    for name in decs:            # warm-up: graph capture, module loading
        run(name)
    res = {name: [] for name in decs}
    for _ in range(a.reps):
        for name in decs:
            r = run(name)
            res[name].append(r)
            print(json.dumps(r), flush=True)
    med = {name: {key: statistics.median(x[key] for x in rs) for key in ("us_per_step", "generate_ms", "tokens_per_s", "begin_ms")}
           for name, rs in res.items()}
    print(json.dumps(dict(summary=True, prompts=a.prompts, samples=nb, rows=rows, length=a.length, reps=a.reps, median=med,
                          stochastic_over_beam_step=med["stochastic"]["us_per_step"] / med["beam"]["us_per_step"])), flush=True)

    # ---- the launches alone, on the buffers the last stochastic generation left, at a free lyric column
    dec = decs["stochastic"][0]
    eng, sh = dec.eng, dec.eng.sh
    Vc, sent = min(sh.V, 13317), sh.msl + 2
    posd = torch.zeros(2, dtype=torch.int32, device="cuda")
    posd[0] = sh.P + 100                                    # lyric index 101: column 13 of its line
    launches = 50
    args = (dec.logits, eng.layout.Vpad, Vc, dec.seq, posd[0:1], sh.P, sent, 1.1, 1.5, nb, dec.cand_val, dec.cand_id)

    def gumbel_candidates():
        hip.decode_gumbel_candidates(*args, dec.cand_g, dec.scores, dec.gum, dec.row_seed, dec.B, dec._no_src)

    def beam_candidates():
        hip.decode_beam_candidates(*args, dec.B)

    def gumbel_merge():
        hip.decode_gumbel_merge(dec.cand_val, dec.cand_id, dec.cand_g, dec.scores, dec.gum, dec.seq, dec.keep, dec.rows, posd[0:1], sh.P,
                                sent, nb, a.prompts, pos_next=posd[1:2])

    def beam_merge():
        hip.decode_beam_merge(dec.cand_val, dec.cand_id, dec.scores, dec.seq, dec.keep, dec.rows, posd[0:1], sh.P, sent, nb, a.prompts,
                              pos_next=posd[1:2])

    def timed(fn):
        dec.scores.zero_()                                  # every row live, whatever the launches before left
        dec.gum.zero_()
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(launches):
                fn()
        g.replay()
        torch.cuda.synchronize()
        out = []
        for _ in range(max(a.reps, 3)):
            dec.scores.zero_()
            dec.gum.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            out.append(1e3 * e0.elapsed_time(e1) / (20 * launches))
        return statistics.median(out)

    us = dict(gumbel_candidates_us=timed(gumbel_candidates), beam_candidates_us=timed(beam_candidates))
    gumbel_candidates()                                     # (the merges read a full set of tables)
    us.update(gumbel_merge_us=timed(gumbel_merge), beam_merge_us=timed(beam_merge))
    print(json.dumps(dict(launches=True, rows=rows, V=Vc, position=int(posd[0]), **us)), flush=True)


if __name__ == "__main__":
    main()
