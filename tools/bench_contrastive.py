"""Contrastive-search token step against the beam-search token step on the same prompts (12-layer base model, bf16, full length),
and the two new launches on their own.

    python tools/bench_contrastive.py [--prompts 64] [--top-k 4] [--alpha 0.6] [--length 220] [--reps 5]

In one process it alternates ContrastiveDecoder (prompts x top_k rows) and BeamDecoder (prompts, top_k beams: the same rows, the
same prompts), both graph-replayed, and reports per decoder what tools/bench_beam.py reports: us per token step (the replayed
steps of a generation between two device synchronisations; begin() is timed apart), the whole generate() time, tokens/s.  One JSON
line per decoder and rep, then a summary line with the medians.  The beam decoder's launches are the ones tools/bench_beam.py
times with the same model and prompts, so that tool on another commit gives that commit's beam step.
Then mmtg_decode_contrastive_sim and mmtg_decode_contrastive_merge alone, on the decoder's own buffers as the generation left
them, at context lengths 1, 118 and 236 (a decoder of max_len 237): 50 launches captured in one graph, replayed, device events
around the replays; one JSON line per context length with us per launch and, for the similarity, the context bytes a launch reads
(rows x kept context columns x n_embd x 4) over that time.
For the kernel split, run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_contrastive.py --reps 1`."""
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
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--length", type=int, default=220)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, hip, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import BeamDecoder, ContrastiveDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_contrastive.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    k, rows = a.top_k, a.prompts * a.top_k
    b = synth.make_batch(a.prompts, mcfg, dcfg, V, seed=7)
    batch = {key: torch.from_numpy(np.asarray(v)).cuda() for key, v in b.items() if key not in ("rating", "targets")}
    decs = {"contrastive": (ContrastiveDecoder(model, a.prompts, k, max_len=max(a.length, 237)), dict(penalty_alpha=a.alpha)),
            "beam": (BeamDecoder(model, a.prompts, k, max_len=max(a.length, 237)), {})}
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
    print(json.dumps(dict(summary=True, prompts=a.prompts, top_k=k, alpha=a.alpha, rows=rows, length=a.length, reps=a.reps, median=med,
                          contrastive_over_beam_step=med["contrastive"]["us_per_step"] / med["beam"]["us_per_step"])), flush=True)

    # ---- the two new launches alone, on the buffers the last generation left (every context column holds a unit vector of that run)
    dec = decs["contrastive"][0]
    eng, sh = dec.eng, dec.eng.sh
    pre = "decoder.gpt2.transformer."
    gamma, beta = eng.P(pre + "ln_f.weight"), eng.P(pre + "ln_f.bias")
    dec.Hc[:, a.length:] = dec.Hc[:, :1]                    # (columns past the generation: any unit vectors)
    dec.keep[:, sh.P:] = 1
    posd = torch.zeros(2, dtype=torch.int32, device="cuda")
    launches = 50

    def sim():
        hip.decode_contrastive_sim(dec.h, gamma, beta, sh.eps, dec.Hc, dec.sim, dec.keep, dec.rows, posd[0:1], sh.P, dec.B, sh.D,
                                   scores=dec.scores)

    def merge():
        hip.decode_contrastive_merge(dec.cand_val, dec.cand_id, dec.scores, dec.sim, dec.total, a.alpha, dec.seq, dec.keep, dec.rows,
                                     posd[0:1], sh.P, sh.msl + 2, k, a.prompts, pos_next=posd[1:2])

    def timed(fn):
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
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            out.append(1e3 * e0.elapsed_time(e1) / (20 * launches))
        return statistics.median(out)

    for ctx in (1, 118, 236):
        posd[0] = sh.P + ctx
        dec.scores.zero_()                                  # every row live: every row reads its context
        us_sim = timed(sim)
        dec.scores.zero_()
        us_merge = timed(merge)
        nbytes = rows * ctx * sh.D * 4
        print(json.dumps(dict(launches=True, context=ctx, rows=rows, n_embd=sh.D, sim_us=us_sim, merge_us=us_merge,
                              context_bytes=nbytes, sim_context_gb_per_s=nbytes / us_sim / 1e3)), flush=True)


if __name__ == "__main__":
    main()
