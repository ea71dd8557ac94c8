#!/usr/bin/env python3
"""An eager (use_graph=False) greedy generation at batch 32, 128 positions, full-size bf16 model: the token step's launches are issued
one by one from Python, so the wall time is the host's -- the figure most sensitive to what decode.py does per step.  Prints the
median, the fastest and the slowest of N generations after one warm-up (N = argv[1], default 15), in ms."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mmtg_amd import MMTG, synth
from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
from mmtg_amd.decode import GreedyDecoder

N = int(sys.argv[1]) if len(sys.argv) > 1 else 15
S, V, B, Ln = 5, 13317, 32, 128
mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16", token_table=synth.make_token_table(V, seed=2))
model.reset_parameters(seed=0)
model.to("cuda").eval()
nb = synth.make_batch(B, mcfg, dcfg, V, seed=7)
batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in nb.items() if k not in ("rating", "targets")}
dec = GreedyDecoder(model, max_batch=B, max_len=Ln, use_graph=False)
first = dec.generate(batch, Ln, temperature=1.1, repitition_penalty=1.5)
times = []
for _ in range(N):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids = dec.generate(batch, Ln, temperature=1.1, repitition_penalty=1.5)
    torch.cuda.synchronize()
    times.append(1e3 * (time.perf_counter() - t0))
assert torch.equal(ids, first)
times.sort()
print("eager generation, batch %d, %d positions: median %.3f ms, fastest %.3f, slowest %.3f over %d" % (B, Ln, times[N // 2], times[0], times[-1], N))
