"""Child process of tests/test_accum_gpu.py: one rank, MMTG_FORCE_DDP=1, joins the RCCL ("nccl") process group BEFORE touching the GPU
in any other way, then runs two windows of three micro-steps through the bucketed exchange -- counting torch.distributed's
all-reduces per CALL of step() -- and the same two windows on a non-distributed trainer from the same state.

    python tests/accum_ddp_worker.py <out.pt>        (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* from the env)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

K = 3


def main():
    out = sys.argv[1]
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    assert world == 1 and os.environ.get("MMTG_FORCE_DDP")
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)     # first GPU touch of this process
    torch.cuda.set_device(dev)
    from ddp_worker import build
    from mmtg_amd import synth
    from mmtg_amd.trainer import MMTGTrainer
    res = {"backend": dist.get_backend()}
    try:
        pairs = []
        for distributed in (True, False):
            model, mcfg, dcfg, V = build("bf16", 0.1, dev)
            tr = MMTGTrainer(model, lr=1e-3, alpha=0.2, distributed=distributed, bucket_mb=8.0, accumulation_steps=K)
            tr.eng.drop_seed = 4242                     # same dropout masks in both runs
            pairs.append((model, tr))
        red = pairs[0][1].reducer
        assert red is not None and red.active and len(red.buckets) > 3 and pairs[1][1].reducer is None
        res["buckets"] = len(red.buckets)
        # unequal micro-batches, one of them a single row
        rows = [(0, 3), (3, 4), (4, 6)]
        nb = synth.make_batch(6, mcfg, dcfg, V, seed=7)
        full = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in nb.items()}
        per_call, hooks, params = [], [], {True: [], False: []}
        orig, orig_bwd = dist.all_reduce, pairs[0][1].eng.backward

        def counting(t, *a, **k):
            per_call[-1].append(t.numel())
            return orig(t, *a, **k)

        def backward(*a, **k):
            hooks.append(pairs[0][1].eng.bucket_hook is not None)
            return orig_bwd(*a, **k)

        pairs[0][1].eng.backward = backward
        for window in range(2):
            for (model, tr), distributed in zip(pairs, (True, False)):
                for lo, hi in rows:
                    mb = {k: v[lo:hi] for k, v in full.items()}
                    if distributed:
                        per_call.append([])
                        dist.all_reduce = counting
                        try:
                            tr.step(mb, stage=3)
                        finally:
                            dist.all_reduce = orig
                    else:
                        tr.step(mb, stage=3)
                torch.cuda.synchronize()
                assert tr.micro_step == 0 and tr.sched_step == window + 1 and tr.eng.step_count == window + 1
                params[distributed].append(model._flat.detach().cpu().clone())
        res.update(per_call=per_call, hooks=hooks, params=params, count=float(pairs[0][1]._count.item()), layout_total=pairs[0][0].layout.total)
        res["ok"] = True
    finally:
        torch.save(res, out + ".r%d" % rank)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
