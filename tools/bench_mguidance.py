"""Per-modality guidance (ModalityGuidedDecoder): what a token step with two and with three negatives costs, and which form of the
combine to launch (12-layer base model, bf16, 220 positions, graph replay).

    python tools/bench_mguidance.py [--length 220] [--reps 3] [--kernel-reps 7] [--launches 200]

In one process, alternating within every rep, medians reported (measuring guide: same box, alternating, medians):

  steps    us per replayed token step (the replayed steps between two device synchronisations; begin() apart) of a sampled generation
           (temperature 1.1, top_k 10, top_p 0.7, penalty 1.5) of
             * three:               ModalityGuidedDecoder, 85 prompts beside 2 negatives each (255 rows), scales i 3, t 1.5;
             * four:                ModalityGuidedDecoder, 64 prompts beside 3 negatives each (256 rows), scales u 2, i 3, t 1.5;
             * guided:              GuidedDecoder, 128 prompts beside their negatives (256 rows), guidance_scale 3;
             * plain / plain_again: GreedyDecoder at 256 rows, twice -- the distance between the two medians is the spread between
                                    equal cases of this run.
  combine  us per launch of the combine alone, `--launches` back-to-back launches between two events (the inputs stay in the caches
           from launch to launch, as the head's product leaves them in the step), V = 13317, rows Vpad apart:
             * resident_3x85 / reread_3x85, resident_4x64 / reread_4x64: mmtg_decode_guidance_multi_form, both forms;
             * two_row_128: mmtg_decode_guidance at 128 pairs; two_row_128_again gives the spread.
           and the achieved bytes/s over the 4 K N V input bytes plus the 4 N V output bytes.
  launches the C entries one eager token step with the head calls, in order, for the plain, the guided and the two new decoders.

One JSON line per measurement, then a summary line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Recorder:
    """Stands in for the loaded library and notes the name of every entry called through it while `log` is a list."""

    def __init__(self, lib):
        self._lib, self.log = lib, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if self.log is None or not name.startswith("mmtg_") or name == "mmtg_last_error":
            return fn

        def call(*a):
            self.log.append(name[5:])
            return fn(*a)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=220)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmtg_amd import MMTG, hip, synth
    from mmtg_amd.configs import data_config, gpt2_config, make_model_cfgs
    from mmtg_amd.decode import GreedyDecoder, GuidedDecoder, ModalityGuidedDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_mguidance.py needs the GPU")
    S, V = 5, 13317
    mcfg, dcfg = make_model_cfgs(seq_len=S), data_config(seq_len=S)
    model = MMTG(mcfg, dcfg, V, gpt2_config=gpt2_config(n_layer=12, vocab_size=V), compute_dtype="bf16",
                 token_table=synth.make_token_table(V, seed=2))
    model.reset_parameters(seed=0)
    model.to("cuda").eval()
    raw = synth.make_batch(256, mcfg, dcfg, V, seed=7)
    batch = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in raw.items() if k not in ("rating", "targets")}

    def without(b, keys):
        return {k: (torch.zeros_like(v) if k in keys else v) for k, v in b.items()}
    zero = {"u": ("img_embs", "r_embs"), "i": ("img_embs",), "t": ("r_embs",)}
    kw = dict(temperature=1.1, repitition_penalty=1.5, top_k=10, top_p=0.7)
    setups = {"three": (85, ("i", "t"), (3.0, 1.5)), "four": (64, ("u", "i", "t"), (2.0, 3.0, 1.5))}
    decs = {name: ModalityGuidedDecoder(model, n, 1 + len(br), max_len=a.length) for name, (n, br, _) in setups.items()}
    decs["guided"] = GuidedDecoder(model, 128, max_len=a.length)
    decs["plain"] = decs["plain_again"] = GreedyDecoder(model, 256, max_len=a.length)
    cases = ("three", "four", "guided", "plain", "plain_again")

    def begin(name, gen):
        dec = decs[name]
        if name in setups:
            n, br, sc = setups[name]
            prompts = {k: v[:n] for k, v in batch.items()}
            return dec.begin(prompts, [without(prompts, zero[b]) for b in br], a.length, br, sc, generator=gen, **kw)
        if name == "guided":
            prompts = {k: v[:128] for k, v in batch.items()}
            return dec.begin(prompts, without(prompts, zero["u"]), a.length, 3.0, generator=gen, **kw)
        return dec.begin(batch, a.length, generator=gen, **kw)

    def step(name):
        dec = decs[name]
        torch.cuda.synchronize()
        n_steps = begin(name, torch.Generator(device="cuda").manual_seed(3))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for pos in range(dec.first_pos, n_steps):
            dec.step_at(pos)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steps = n_steps - dec.first_pos
        return dict(kind="step", case=name, rows=dec.B, length=a.length, steps=steps, us_per_step=1e6 * (t2 - t1) / steps)

    for name in cases[:4]:                  # warm-up: graph capture, module loading
        step(name)
    res = {name: [] for name in cases}
    for _ in range(a.reps):
        for name in cases:
            r = step(name)
            res[name].append(r["us_per_step"])
            print(json.dumps(r), flush=True)
    med = {name: statistics.median(v) for name, v in res.items()}

    # ---- the combine alone
    Vpad = decs["plain"].eng.layout.Vpad
    logits = torch.randn(256, Vpad, device="cuda") * 4.0
    out = torch.zeros(128, Vpad, device="cuda")
    kernels = {}
    for K, N, sc in ((3, 85, (3.0, 1.5)), (4, 64, (2.0, 3.0, 1.5))):
        for form in ("resident", "reread"):
            kernels["%s_%dx%d" % (form, K, N)] = (lambda N=N, sc=sc, form=form: hip.decode_guidance_multi(logits, Vpad, V, sc, out, N, form=form),
                                                  4.0 * (K + 1) * N * V)
    two = (lambda: hip.decode_guidance(logits, logits[128:], Vpad, V, 3.0, out, 128), 4.0 * 3 * 128 * V)
    kernels["two_row_128"] = kernels["two_row_128_again"] = two
    kres = {name: [] for name in kernels}
    for rep in range(a.kernel_reps + 1):
        for name, (launch, nbytes) in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            launch()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / a.launches
            if rep:                         # (the first round warms up)
                kres[name].append(us)
                print(json.dumps(dict(kind="combine", case=name, us_per_launch=us, gbytes_per_s=nbytes / us * 1e-3)), flush=True)
    kmed = {name: statistics.median(v) for name, v in kres.items()}

    # ---- the launch lists
    rec = Recorder(hip.lib())
    hip._lib = rec
    lists = {}
    try:
        for name in ("plain", "guided", "three", "four"):
            dec = decs[name]
            n_steps = begin(name, torch.Generator(device="cuda").manual_seed(3))
            saved, dec.use_graph = dec.use_graph, False
            try:
                rec.log = []
                with_head = dec.step_at(dec.first_pos)
                lists[name] = dict(with_head=bool(with_head), entries=rec.log)
            finally:
                rec.log, dec.use_graph = None, saved
            torch.cuda.synchronize()
            print(json.dumps(dict(kind="launches", case=name, **lists[name])), flush=True)
    finally:
        hip._lib = rec._lib
    tail = {name: v["entries"][len(lists["plain"]["entries"]) - 1:] for name, v in lists.items()}
    print(json.dumps(dict(summary=True, length=a.length, reps=a.reps, median_us_per_step=med,
                          minus_plain_us={n: med[n] - med["plain"] for n in ("three", "four", "guided")},
                          spread_between_equal_cases_us=abs(med["plain_again"] - med["plain"]),
                          combine_median_us=kmed, combine_gbytes_per_s={n: kernels[n][1] / kmed[n] * 1e-3 for n in kmed},
                          combine_spread_us=abs(kmed["two_row_128_again"] - kmed["two_row_128"]),
                          step_tail_entries=tail, describe={n: decs[n].describe() for n in ("three", "four", "guided")})), flush=True)


if __name__ == "__main__":
    main()
