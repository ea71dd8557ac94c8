"""Fused training step: the hot loop of the reference's src/train.py:177-200 as one
sequence of HIP kernel launches without host synchronisation (losses, the clip coefficient and the
global row count stay on the device).  The one exception is the in-trainer curriculum filter of
stages 1 / 2 on DEVICE ratings, which reads the selection back once per step; hand the ratings
over on the host as well (``batch["rating_host"]``) or filter in the loader (``DeviceLoader``)
and the step is sync-free in every stage.

    filter rows by curriculum stage  -> forward -> MyLoss (+ alpha * KL) -> backward
    -> bucketed RCCL all-reduce (overlapped) -> clip_grad_norm_(1.0) + AdamW + LR schedule

Optimizer semantics are transformers.AdamW as train.py:137 constructs it
(betas .9/.999, eps 1e-6, weight_decay 0, bias-corrected) with
get_linear_schedule_with_warmup (train.py:146-148).
"""
from __future__ import annotations

import contextlib
import copy
import os

import torch

from .ddp import GradReducer


def curriculum_filter(ratings, stage):
    """Row selection + order of train.py:178-183 (negatives first)."""
    r = torch.as_tensor(ratings)
    if stage == 1:
        return torch.cat([torch.where(r < 2)[0], torch.where(r > 4)[0]])
    if stage == 2:
        return torch.cat([torch.where(r < 3)[0], torch.where(r > 3)[0]])
    return torch.arange(len(r), device=r.device)


def linear_schedule(step, warmup, total):
    """LR multiplier of get_linear_schedule_with_warmup after `step` scheduler steps."""
    if step < warmup:
        return step / max(1, warmup)
    return max(0.0, (total - step) / max(1, total - warmup))


_LOGITS_F32 = bool(os.environ.get("MMTG_LOGITS_F32"))     # A/B switch: fp32 logits in the bf16 trainer too

NO_EXPERIENCE = (1.0, 0.0, 0.0)         # exp_drop of a forward on generate.without_experience of its batch


def _check_scales(scales):
    """The scales of the guided validation loss as a list of floats: 1 .. 8 of them, each as constraints.check_guidance takes it."""
    from .constraints import check_guidance
    from .hip import GUIDED_MAX_SCALES
    if isinstance(scales, (str, bytes)):
        raise ValueError("scales must be a sequence of 1 .. %d guidance scales, got %r" % (GUIDED_MAX_SCALES, scales))
    try:
        scales = list(scales)
    except TypeError:
        raise ValueError("scales must be a sequence of 1 .. %d guidance scales, got %r" % (GUIDED_MAX_SCALES, scales)) from None
    if not 1 <= len(scales) <= GUIDED_MAX_SCALES:
        raise ValueError("scales must hold 1 .. %d guidance scales, got %d" % (GUIDED_MAX_SCALES, len(scales)))
    return [check_guidance(s) for s in scales]


def _check_scale_triples(scales):
    """The scales of the per-modality guided validation loss as a list of float triples (guidance_scale, image_guidance_scale,
    text_guidance_scale): 1 .. 8 of them, each through constraints.check_modality_guidance, whose messages name the decoder's arguments."""
    from .constraints import check_guidance, check_modality_guidance
    from .hip import GUIDED_MAX_SCALES
    msg = "scales must be a sequence of 1 .. %d (guidance_scale, image_guidance_scale, text_guidance_scale) triples, got %r" % (
        GUIDED_MAX_SCALES, scales)
    if isinstance(scales, (str, bytes)):
        raise ValueError(msg)
    try:
        scales = list(scales)
    except TypeError:
        raise ValueError(msg) from None
    if not 1 <= len(scales) <= GUIDED_MAX_SCALES:
        raise ValueError("scales must hold 1 .. %d triples of guidance scales, got %d" % (GUIDED_MAX_SCALES, len(scales)))
    out = []
    for t in scales:
        if isinstance(t, (str, bytes)):
            raise ValueError(msg)
        try:
            t = tuple(t)
        except TypeError:
            raise ValueError(msg) from None
        if len(t) != 3:
            raise ValueError(msg)
        check_modality_guidance(*t)
        out.append(tuple(check_guidance(s) for s in t))
    return out


def best_scale(result):
    """The entry of result['scales'] with the lowest result['ce'] (the first of equal minima), for the result of
    MMTGTrainer.evaluate_guided (a float) or evaluate_modality_guided (a triple).  A result over no rows, or one with a ce that is
    not finite, raises a ValueError: there is nothing to choose by."""
    import math
    scales, ce = list(result["scales"]), [float(v) for v in result["ce"]]
    if int(result["rows"]) == 0:
        raise ValueError("best_scale: the result covers no rows (rows == 0)")
    if len(scales) != len(ce) or not ce:
        raise ValueError("best_scale: %d scales beside %d ce values" % (len(scales), len(ce)))
    if not all(math.isfinite(v) for v in ce):
        raise ValueError("best_scale: ce must be finite, got %r" % (ce,))
    return scales[min(range(len(ce)), key=ce.__getitem__)]


def _check_experience_drop(value):
    """MMTGTrainer's experience_drop as the triple (p_both, p_img, p_txt): a float p in [0, 1] is (p, 0, 0); a sequence of three
    floats, each in [0, 1] with a sum of at most 1, is itself.  Anything else raises a ValueError that names the argument."""
    msg = "experience_drop must be a float in [0, 1] or three floats (p_both, p_img, p_txt) in [0, 1] with a sum <= 1, got %r" % (value,)
    real = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and 0.0 <= v <= 1.0       # (NaN fails the comparison)
    if real(value):
        return (float(value), 0.0, 0.0)
    if isinstance(value, (str, bytes, bool, int, float)) or value is None:
        raise ValueError(msg)
    try:
        triple = tuple(value)
    except TypeError:
        raise ValueError(msg) from None
    if len(triple) != 3 or not all(real(v) for v in triple) or sum(float(v) for v in triple) > 1.0:
        raise ValueError(msg)
    return tuple(float(v) for v in triple)


class MMTGTrainer:
    def __init__(self, model, lr=1e-5, alpha=0.0, max_norm=1.0, betas=(0.9, 0.999), eps=1e-6,
                 weight_decay=0.0, warmup_steps=0, total_steps=None, distributed=False, bucket_mb=64.0,
                 lm_weight=0.0, param_groups=None, accumulation_steps=1, ema_decay=None, ema_warmup=True,
                 ul_weight=0.0, ul_exclude_ids=None, cl_weight=0.0, cl_margin=0.5, experience_drop=0.0,
                 distill_weight=0.0, distill_teacher=None, distill_scale=1.0):
        """distill_weight: weight of the distillation term (the rule is stated in include/mmtg_hip.h): per lyric row the Kullback-
        Leibler divergence KL(q || p) of the model's distribution p from the teacher's q, so the objective becomes
        ... + distill_weight * kd, normalised per sample.  distill_teacher: a second MMTG model on the same device, of any compute
        mode, with the student's vocabulary and topic length; it runs in eval mode, is never updated and is no part of state_dict()
        or of a checkpoint.  The trained model itself is refused (its forward would overwrite the step's activations): pass
        copy.deepcopy(model).  distill_scale: q = softmax(lu + s (lc - lu)) of the teacher's logits for the batch (lc) and for the
        batch without its images and texts (lu) -- the distribution generate_samples(guidance_scale=s) draws from, so that a model
        trained towards it decodes plainly, at full batch and in every decoder, what guidance gave (choose s with evaluate_guided).
        At the default 1.0 the teacher runs one forward per micro-step and q = softmax(lc): ordinary knowledge distillation, for
        example of a 12-layer teacher into a 6-layer student; at any other scale it runs two.  step() and evaluate_batch() then also
        return 'kd', the unweighted term.  0.0 (the default) launches nothing new and keeps no buffer.  Not together with ul_weight
        (both replace the d(logits) kernel) or experience_drop (a row whose experience was dropped must not be pulled towards the
        guided distribution of the full prompt).  Only the fused step takes the term.
        experience_drop: the training side of classifier-free guidance (generate_samples(guidance_scale=...), GuidedDecoder).  A
        float p in [0, 1] replaces, per sample and with probability p, the images and texts of the experience by zeros -- exactly what
        generate.without_experience feeds the decoders as the default negative -- so that the branch guidance subtracts is a
        distribution the model was trained on.  A sequence (p_both, p_img, p_txt), each in [0, 1] and summing to at most 1, also drops
        the images alone or the texts alone; the three events are disjoint (one hash per sample, mmtg_experience_drop in
        include/mmtg_hip.h).  Applied in step() while the model is in training mode, the gate of the dropout sites; a dropped row takes
        part in every term of the objective unchanged.  step() then also returns 'experience_drop', the int32 codes of the local rows
        (bit 0: images dropped, bit 1: texts dropped).  0.0 (the default) launches nothing new and keeps no buffer.  Only the fused
        step takes it.
        cl_weight: weight of the contrastive token loss on the last-layer states (SimCTG, Su et al., 2022; the rule is stated in
        include/mmtg_hip.h): within one sample the ln_f outputs of different kept lyric positions are pushed apart until their cosine
        is below 1 - cl_margin, which is what generate_contrastive's degeneration penalty reads.  The objective becomes
        ... + cl_weight * cl, normalised per sample (not by SimCTG's batch-global pair count), so a window of micro-batches and a
        data-parallel shard equal the big batch.  0.0 (the default) runs exactly the launches it always did; > 0 adds two entries
        (mmtg_cl_fwd after the loss, mmtg_cl_bwd between the LM head's backward and ln_f's).  cl_margin: a float in (0, 1], the paper's
        rho.  Only the fused step takes the term.
        ul_weight: weight of the token-level unlikelihood term on repeated lyric tokens (Welleck et al., 2019; the rule is stated
        in include/mmtg_hip.h): at every lyric position the characters the lyric has already used are pushed down, so the objective
        becomes MyLoss + alpha * KL (+ lm_weight * LM) + ul_weight * ul.  0.0 (the default) is the reference's objective and runs
        exactly the launches it always did; > 0 adds two small launches and replaces the d(logits) kernel by the one that carries the
        term.  ul_exclude_ids: at most 32 ids that are never pushed down, None = PAD and the ids the decoders ban
        (0,) + constraints.BANNED -- they repeat by the slot format, not by the model's choice; with another tokenizer pass
        tokenizer.convert_tokens_to_ids of its own format tokens.  Only the fused step takes the term; the drop-in autograd path
        (mmtg_amd.loss.MyLoss) is the reference's loss.
        accumulation_steps: calls of step() per optimizer step (a window of micro-batches, see step()).
        ema_decay: None (no average: no buffer, no launch) or a float in (0, 1), the decay of an exponential moving average of
        the parameters kept next to the masters and updated once per optimizer step (see _close_end); ema_warmup: the decay of
        update t (from 0) is min(ema_decay, (1 + t) / (10 + t)), so that the first steps do not pin the average to the initial
        weights.  In a data-parallel group every rank keeps its own average and nothing is exchanged: the parameters are identical
        across ranks after every step, and so are the averages.  averaged_weights() / evaluate(averaged=True) /
        ema_state_dict() / save_checkpoint(averaged=True) read it.
        param_groups: a list of specs as mmtg_amd.param_groups takes them (fnmatch patterns on the state-dict keys; per group
        `lr_scale`, `weight_decay`, `frozen`).  `lr` and the schedule stay the base rate, groups scale it; None is the single
        group of the reference."""
        if type(accumulation_steps) is not int or accumulation_steps < 1:
            raise ValueError("accumulation_steps must be an int of at least 1, got %r" % (accumulation_steps,))
        if ema_decay is not None and not (isinstance(ema_decay, float) and 0.0 < ema_decay < 1.0):
            raise ValueError("ema_decay must be None or a float in (0, 1), got %r" % (ema_decay,))
        if isinstance(ul_weight, bool) or not isinstance(ul_weight, (int, float)) or not (0.0 <= ul_weight < float("inf")):
            raise ValueError("ul_weight must be a finite float >= 0, got %r" % (ul_weight,))
        if ul_exclude_ids is None:
            from .constraints import BANNED
            ul_exclude_ids = (0,) + tuple(BANNED)
        try:
            ul_exclude_ids = tuple(ul_exclude_ids)
        except TypeError:
            raise ValueError("ul_exclude_ids must be None or a sequence of at most 32 non-negative ints, got %r" % (ul_exclude_ids,)) from None
        if len(ul_exclude_ids) > 32 or any(type(i) is not int or i < 0 for i in ul_exclude_ids):
            raise ValueError("ul_exclude_ids must be None or a sequence of at most 32 non-negative ints, got %r" % (ul_exclude_ids,))
        self.ul_weight, self.ul_exclude_ids = float(ul_weight), ul_exclude_ids
        if isinstance(cl_weight, bool) or not isinstance(cl_weight, (int, float)) or not (0.0 <= cl_weight < float("inf")):
            raise ValueError("cl_weight must be a finite float >= 0, got %r" % (cl_weight,))
        if isinstance(cl_margin, bool) or not isinstance(cl_margin, (int, float)) or not (0.0 < cl_margin <= 1.0):
            raise ValueError("cl_margin must be a float in (0, 1], got %r" % (cl_margin,))
        self.cl_weight, self.cl_margin = float(cl_weight), float(cl_margin)
        self.experience_drop = _check_experience_drop(experience_drop)
        self._exp_drop_on = any(p > 0.0 for p in self.experience_drop)
        if isinstance(distill_weight, bool) or not isinstance(distill_weight, (int, float)) or not (0.0 <= distill_weight < float("inf")):
            raise ValueError("distill_weight must be a finite float >= 0, got %r" % (distill_weight,))
        from .constraints import check_guidance
        try:
            self.distill_scale = check_guidance(distill_scale)
        except ValueError as e:
            raise ValueError("distill_scale: %s" % e) from None
        self.distill_weight = float(distill_weight)
        if self.distill_weight > 0.0 and distill_teacher is None:
            raise ValueError("distill_weight = %g needs distill_teacher: the term is measured against a teacher's logits" % self.distill_weight)
        if self.distill_weight == 0.0 and distill_teacher is not None:
            raise ValueError("distill_teacher with distill_weight = 0: the teacher would run for nothing; pass a weight > 0 or no teacher")
        if self.distill_weight > 0.0 and self.ul_weight > 0.0:
            raise ValueError("distill_weight > 0 with ul_weight > 0: both terms replace the d(logits) kernel and no kernel carries both")
        if self.distill_weight > 0.0 and self._exp_drop_on:
            raise ValueError("distill_weight > 0 with experience_drop: a row whose experience was dropped would be pulled towards the "
                             "teacher's distribution for the full prompt")
        if distill_teacher is not None and distill_teacher is model:
            raise ValueError("distill_teacher is the trained model itself: its forward would overwrite the step's activations; "
                             "pass a copy (copy.deepcopy(model))")
        self.distill_teacher = distill_teacher
        self.accumulation_steps = accumulation_steps
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema_updates = 0                    # updates of the average made so far
        self._averaged = False                  # inside averaged_weights(): master and average are exchanged
        self.model = model
        self.eng = model.engine()
        if self.ul_weight > 0.0:
            self.eng.set_ul_exclude(self.ul_exclude_ids)         # uploaded once, here
        self.teng = None
        if distill_teacher is not None:
            self.teng = distill_teacher.engine()
            if self.teng is self.eng:
                raise ValueError("distill_teacher shares the trained model's engine: pass a copy (copy.deepcopy(model))")
            if self.teng.dev != self.eng.dev:
                raise ValueError("distill_teacher is on %s, the model on %s" % (self.teng.dev, self.eng.dev))
            if (self.teng.sh.V, self.teng.sh.P) != (self.eng.sh.V, self.eng.sh.P):
                raise ValueError("distill_teacher has V = %d, P = %d; the model has V = %d, P = %d: the two distributions must be over "
                                 "one vocabulary on the same rows" % (self.teng.sh.V, self.teng.sh.P, self.eng.sh.V, self.eng.sh.P))
        self.group_plan = self.groups = None
        if param_groups is not None:
            from . import hip
            from .param_groups import build_param_groups
            self.group_plan = build_param_groups(self.eng.layout, param_groups, weight_decay)
            self.groups = hip.GroupTable(self.group_plan, self.eng.dev)       # the segment table is uploaded once, here
        self.lr, self.alpha, self.max_norm = lr, alpha, max_norm
        self.betas, self.eps, self.wd = betas, eps, weight_decay
        self.warmup, self.total = warmup_steps, total_steps
        self.sched_step = 0
        self.lm_weight = lm_weight
        self.reducer = GradReducer(self.eng.layout, bucket_mb) if distributed else None
        self._count = None
        self.measure_finish, self.finish_events = False, []
        # (the exchange belongs to a window's closing backward: only there are the packs it passes final, see _step)
        self._hook = None if self.reducer is None else (lambda pack: self.reducer.on_pack_ready(self.eng.grad, pack))
        if self.reducer is not None:
            self.eng.bucket_hook = self._hook if accumulation_steps == 1 else None
        self.window = None          # device scalars of the last closed window (see step)
        self._micro = self._rows = 0            # calls / local rows of the open window
        self._bwd_ran = False                   # a backward of the open window has run (the buffer is zeroed before the first)
        self._wacc = self._tune_ev = None
        # Self-tuning CU reservation (round 5): a multi-rank GPU run whose environment does not pin MMTG_DDP_GEMM_CUS spends its
        # first steps under each candidate (ddp.BUDGET_CANDIDATES: 0 / 16 / 32 CUs left to the RCCL kernels; TUNE_STEPS real
        # optimisation steps each, the first of every candidate untimed), then all ranks agree on the fastest through one MAX
        # all-reduce of the timings (ddp.agree_on_budget) -- whether RCCL holds CUs beside the backward depends on the node
        # (profiles/r04_v1_ddp_cu_contention_one_gpu.txt priced a wrong guess at 5 % of the step either way).
        from . import ddp as _ddp
        self._tune = None
        self.budget_report = None
        if (self.reducer is not None and self.reducer.world > 1 and self.eng.dev.type == "cuda" and not _ddp.cu_budget_fixed()
                and os.environ.get("MMTG_DDP_TUNE", "1") != "0"):
            self._tune = {"cand": list(_ddp.BUDGET_CANDIDATES), "i": 0, "k": 0, "events": [[] for _ in _ddp.BUDGET_CANDIDATES]}
            _ddp.set_chosen_budget(self._tune["cand"][0])

    def current_lr(self):
        if self.total is None:
            return self.lr
        return self.lr * linear_schedule(self.sched_step, self.warmup, self.total)

    # ---- true resume (the reference saves the model only, train.py:212)
    def state_dict(self):
        """Optimizer moments (flat fp32, the engine's parameter order), AdamW step count, scheduler position
        and the dropout counter: together with ``model.state_dict()`` everything a bit-continuing run needs.  Only at a window
        boundary: the gradient sums of an open window are not part of it.  'ema' is None for a trainer without an average, else
        {'decay', 'warmup', 'updates', 'average'} with the flat fp32 average (None before the first step)."""
        self._refuse_averaged("state_dict()")
        if self._micro:
            raise RuntimeError("state_dict() inside an open accumulation window (micro_step = %d of %d): take the checkpoint at a "
                               "boundary, or close the window with flush() first" % (self._micro, self.accumulation_steps))
        eng = self.eng
        return {"format": "mmtg-trainer-1", "layout_total": eng.layout.total,
                "exp_avg": None if eng.opt_m is None else eng.opt_m.detach().cpu().clone(),
                "exp_avg_sq": None if eng.opt_v is None else eng.opt_v.detach().cpu().clone(),
                "step_count": eng.step_count, "sched_step": self.sched_step, "drop_seed": eng.drop_seed,
                # the CU reservation the ranks agreed on (None: not tuned): a resumed run keeps it instead of spending nine steps
                # re-tuning under wall-clock timings (MMTG_DDP_GEMM_CUS pins it from the environment)
                "cu_budget": None if self.budget_report is None else self.budget_report.get("budget_chosen"),
                "ema": None if self.ema_decay is None else {
                    "decay": self.ema_decay, "warmup": self.ema_warmup, "updates": self.ema_updates,
                    "average": None if eng.ema is None else eng.ema.detach().cpu().clone()},
                "hparams": {"lr": self.lr, "alpha": self.alpha, "max_norm": self.max_norm, "betas": tuple(self.betas),
                            "eps": self.eps, "weight_decay": self.wd, "warmup_steps": self.warmup,
                            "total_steps": self.total, "lm_weight": self.lm_weight, "accumulation_steps": self.accumulation_steps,
                            "ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup,
                            "ul_weight": self.ul_weight, "ul_exclude_ids": tuple(self.ul_exclude_ids),
                            "cl_weight": self.cl_weight, "cl_margin": self.cl_margin, "experience_drop": self.experience_drop,
                            "distill_weight": self.distill_weight, "distill_scale": self.distill_scale,
                            # for the record, like the rest: load_state_dict keeps the trainer's own groups as it keeps its own lr
                            "param_groups": None if self.group_plan is None else copy.deepcopy(self.group_plan.specs)}}

    def load_state_dict(self, sd):
        """(accumulation_steps, ul_weight, ul_exclude_ids, cl_weight, cl_margin, experience_drop and the distill_* arguments stay the trainer's own, like lr and the groups; an open window is abandoned)
        A trainer with an average takes 'average' and 'updates' from the dict; from a dict without an average (an older
        checkpoint, a run that kept none) the average is dropped and restarts from the loaded weights at the next step.  The decay
        and the warm-up rule stay the trainer's own; a trainer without an average ignores the key."""
        self._refuse_averaged("load_state_dict()")
        eng = self.eng
        if sd.get("format") != "mmtg-trainer-1" or sd.get("layout_total") != eng.layout.total:
            raise ValueError("trainer state of a different model layout (%s, %s parameters; this model has %d)"
                             % (sd.get("format"), sd.get("layout_total"), eng.layout.total))
        if self.ema_decay is not None:
            rec = sd.get("ema") or {}
            avg = rec.get("average")
            if avg is not None and avg.numel() != eng.layout.total:
                raise ValueError("trainer state with an average of %d elements; this model's flat buffer has %d"
                                 % (avg.numel(), eng.layout.total))
            eng.ema = None if avg is None else avg.to(eng.dev, torch.float32).reshape(-1).clone()
            self.ema_updates = 0 if avg is None else int(rec.get("updates", 0))
        for name, key in (("opt_m", "exp_avg"), ("opt_v", "exp_avg_sq")):
            v = sd[key]
            setattr(eng, name, None if v is None else v.to(eng.dev, torch.float32).clone())
        eng.step_count, self.sched_step, eng.drop_seed = int(sd["step_count"]), int(sd["sched_step"]), int(sd["drop_seed"])
        self.reset_window()
        if sd.get("cu_budget") is not None and self._tune is not None:
            from . import ddp as _ddp
            _ddp.set_chosen_budget(int(sd["cu_budget"]))
            self.budget_report = {"budget_chosen": int(sd["cu_budget"]), "source": "checkpoint"}
            self._tune = None

    def step(self, batch, stage=3, filter_rows=True):
        """One optimisation step; returns device scalars (no host sync) {'loss','lm_loss','kl'} of the LOCAL rows (with ul_weight > 0
        also 'ul', the unweighted unlikelihood term; with cl_weight > 0 also 'cl', the unweighted contrastive term; with
        distill_weight > 0 also 'kd', the unweighted distillation term; with experience_drop on and the model in training mode also 'experience_drop', the device int32 codes of the local rows).
        Returns None when the stage filter leaves no rows on a single rank (train.py:184-185); in a data-parallel
        group a rank without rows still takes part in the exchange and in the (identical) optimizer step.

        Scaling.  The backward produces the SUM over local rows of the per-row gradients (loss coefficient n_local /
        n_local, KL weight alpha * n_local); the global row count travels as a DEVICE scalar -- all-reduced next to the
        gradient buckets when distributed, never read by the host -- and the clip + AdamW kernel divides by it.  Single
        GPU and data-parallel steps therefore run the same arithmetic, and unequal shards after curriculum filtering
        give the single-GPU global mean.

        One documented difference: when EVERY rank of a multi-rank group is filtered to zero rows, the AdamW kernel sees a
        global count of 0 and leaves parameters and moments untouched, but the host -- which never reads the count --
        still advances the Adam step (bias correction) and the LR schedule by one.  A single process `continue`s before
        either counter moves (train.py:184-185).  Shards of a shuffled global batch that are ALL empty after the stage
        filter do not occur with the released data (every rating occurs in every batch of 64+ rows); the price of the
        exact behaviour would be a host read of the all-reduced count every step.  The average (ema_decay) follows the same rule:
        its kernel reads the count and leaves the average untouched, while the host advances `ema_updates` -- and with it the
        warm-up of the decay -- by one.

        Gradient accumulation.  With accumulation_steps = k > 1 a call is a MICRO-step and k consecutive calls -- counted in calls,
        not rows, so every rank of a group closes at the same call -- are a window: the buffer is zeroed once, before the window's
        first backward (which overwrites, as the single step's does); the later backwards add their row sums; the closing call fills
        the row count with the window's total, runs the exchange (the bucket hook is installed for its backward alone: a pack the
        closing backward has passed is final) and ONE clip + AdamW + schedule step.  The same arithmetic as a data-parallel step over
        k ranks.  A call the stage filter empties runs nothing and still counts; a single-rank window without any row moves no
        counter.  `window` then holds the closed window's row-weighted means {'loss','lm_loss','kl'} (device scalars; with k = 1 the
        step's own, valid until the next call) and its local 'rows'.  If a call raises, the window is abandoned (reset_window)."""
        self._refuse_averaged("step()")
        if self._tune is not None and self._micro == 0:      # the tuning books whole windows
            self._tune_ev = torch.cuda.Event(enable_timing=True)
            self._tune_ev.record()
        try:
            out, closed = self._step(batch, stage, filter_rows)
        except BaseException:
            self.reset_window()
            raise
        # (only after a step that RETURNED: the book-keeping ends in a blocking all-reduce, which after an exception on one rank
        #  would turn that rank's error into a hang of the group)
        if closed:
            self._tune_after_window()
        return out

    @property
    def micro_step(self):
        """Calls of step() in the open window; 0 at a window boundary."""
        return self._micro

    def reset_window(self):
        """Abandon the open window: the next call starts a fresh one (zeroing included); collectives in flight are dropped."""
        self._micro = self._rows = 0
        self._bwd_ran = False
        self._tune_ev = None
        if self.reducer is not None:
            self.reducer.reset()

    def flush(self):
        """Close a partial window (the end of an epoch): the exchange and the optimizer step over the rows so far.  True when a
        window was open, False -- and nothing done -- at a boundary."""
        self._refuse_averaged("flush()")
        if not self._micro:
            return False
        red = self.reducer if (self.reducer is not None and self.reducer.active) else None
        try:
            if self._close_begin(red, self._rows):
                self._close_end(red)
            else:
                self._end_window()
        except BaseException:
            self.reset_window()
            raise
        self._tune_after_window()
        return True

    def _tune_after_window(self):
        ev, self._tune_ev = self._tune_ev, None
        if ev is not None and self._tune is not None:
            self._tune_after_step(ev)

    TUNE_STEPS = 3

    def _tune_after_step(self, ev0):
        """Book-keeping of the CU-reservation tuning: one event pair per step; after TUNE_STEPS steps of the last candidate the
        ranks agree (the only host synchronisation of the tuning) and the choice is installed for the rest of the run."""
        from . import ddp as _ddp
        t = self._tune
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        t["events"][t["i"]].append((ev0, ev1))
        t["k"] += 1
        if t["k"] < self.TUNE_STEPS:
            return
        t["k"] = 0
        t["i"] += 1
        if t["i"] < len(t["cand"]):
            _ddp.set_chosen_budget(t["cand"][t["i"]])
            return
        torch.cuda.synchronize()
        ms = [sum(a.elapsed_time(b) for a, b in evs[1:]) / max(1, len(evs) - 1) for evs in t["events"]]
        choice, agreed = _ddp.agree_on_budget(ms, t["cand"], self.reducer.group, device=self.eng.dev)
        _ddp.set_chosen_budget(choice)
        self.budget_report = {"candidates": t["cand"], "ms_per_step_this_rank": [round(x, 3) for x in ms],
                              "ms_per_step_slowest_rank": [round(x, 3) for x in agreed], "budget_chosen": choice,
                              "steps_per_candidate": self.TUNE_STEPS}
        self._tune = None

    def _step(self, batch, stage, filter_rows):
        eng = self.eng
        if filter_rows and stage in (1, 2):
            # The selected row COUNT shapes every launch of the step, so the host has to know it: computed from a host copy
            # of the ratings when the batch carries one ("rating_host", a CPU tensor -- the loader has the ratings on the
            # host anyway; DeviceLoader goes further and filters before the copy) this costs no device synchronisation;
            # from device ratings alone it costs ONE device -> host read per step in stages 1 / 2 (torch.where).
            idx = curriculum_filter(batch["rating_host"] if "rating_host" in batch else batch["rating"], stage)
            batch = {k: v[idx.to(v.device, non_blocking=True)] for k, v in batch.items() if k != "rating_host"}
        elif "rating_host" in batch:
            batch = {k: v for k, v in batch.items() if k != "rating_host"}
        n_local = int(batch["rating"].shape[0]) if "rating" in batch else int(batch["targets"].shape[0])
        red = self.reducer if (self.reducer is not None and self.reducer.active) else None
        self._micro += 1
        closing = self._micro >= self.accumulation_steps
        rows = self._rows + n_local
        if closing and not self._close_begin(red, rows):
            self._end_window()
            return None, True       # nothing to exchange with: no counter moves, as train.py:184-185 `continue`s
        out = None
        if n_local > 0:
            first = not self._bwd_ran
            if first:               # once per window: the later backwards add to what this one writes
                eng.zero_grad((n_local, int(batch["targets"].shape[1])) if "targets" in batch else None)
            if self.distill_weight > 0.0:
                teacher = self._teacher_pass(batch, stage)      # (first: the student's activations are the step's last)
            if self._exp_drop_on and self.model.training:
                # (every micro-step draws its own codes: the step seed advances per forward)
                eng.forward(batch, train_flag=True, training=True, logits_f32=_LOGITS_F32, exp_drop=self.experience_drop)
            else:
                eng.forward(batch, train_flag=True, training=self.model.training, logits_f32=_LOGITS_F32)
            sc = eng.loss(batch["rating"], stage, batch_den=n_local)
            T = eng.act["T"]
            lm_coef = self.lm_weight / (T - 1) if self.lm_weight else 0.0
            if self.ul_weight > 0.0:
                # (every row of the batch takes part whatever its rating; ntok = the lyric columns but the first, as in the loss)
                ul = eng.ul_loss(batch_den=n_local)
                ntok = max(1, int(batch["targets"].shape[1]) - 1)
                dl = eng.loss_backward_ul(float(n_local), lm_coef, self.ul_weight / (ntok * n_local) * float(n_local))
            elif self.distill_weight > 0.0:
                # (every row takes part whatever its rating; the coefficient distill_weight * gscale / (ntok * batch_den))
                kd = eng.distill_loss(*teacher, scale=self.distill_scale, batch_den=n_local)
                ntok = max(1, int(batch["targets"].shape[1]) - 1)
                dl = eng.loss_backward_kd(float(n_local), lm_coef, self.distill_weight / (ntok * n_local) * float(n_local))
            else:
                dl = eng.loss_backward(float(n_local), lm_coef=lm_coef)
            if self.reducer is not None:
                # (before the closing backward the packs are not final; without a hook those backwards overlap their tail, _WGRAD_TAIL)
                eng.bucket_hook = self._hook if closing else None
            eng.wgrad_overwrite = first     # gradients were zeroed above and every weight is written once
            if self.cl_weight > 0.0:
                # (every row of the batch takes part; the coefficient cl_weight * gscale / batch_den with gscale = batch_den = n_local)
                cl = eng.cl_loss(self.cl_margin, batch_den=n_local)
            try:
                if self.cl_weight > 0.0:
                    eng.backward(dl, dkl=self.alpha * n_local, cl_coef=self.cl_weight)
                else:
                    eng.backward(dl, dkl=self.alpha * n_local)
                if first:
                    eng._finish_overwrite_record()
            finally:
                eng.wgrad_overwrite = False
                eng._ow_rec = None
            self._bwd_ran = True
            out = {"loss": sc[0], "lm_loss": sc[1], "kl": eng.act["kl"][0]}
            if self.ul_weight > 0.0:
                out["ul"] = ul[0]
            if self.cl_weight > 0.0:
                out["cl"] = cl[0]
            if self.distill_weight > 0.0:
                out["kd"] = kd[0]
            self._add_to_window(out, sc, n_local)
            if "exp_drop" in eng.act:       # (not a scalar of the window: the step's own rows, valid until the next forward)
                out = dict(out, experience_drop=eng.act["exp_drop"])
        self._rows = rows
        if closing:
            self._close_end(red)
        return out, closing

    def _add_to_window(self, out, sc, n):
        """The window's loss: sum of n_i * v_i on the device, divided by the window's rows when it closes."""
        if self.accumulation_steps == 1:
            self._wacc = out        # the step's own scalars: no launch that today's step does not have
            return
        if self._wacc is None:
            # (slot 3 is 'ul', slot 4 'cl', slot 5 'kd'; a slot whose term is off is neither written nor read)
            self._wacc = torch.empty(6 if self.distill_weight > 0.0 else 5 if self.cl_weight > 0.0 else 4 if self.ul_weight > 0.0 else 3, device=sc.device, dtype=torch.float32)
        if self._rows == 0:         # the window's first rows
            torch.mul(sc[:2], float(n), out=self._wacc[:2])
            torch.mul(out["kl"].reshape(1), float(n), out=self._wacc[2:3])
            if "ul" in out:
                torch.mul(out["ul"].reshape(1), float(n), out=self._wacc[3:4])
            if "cl" in out:
                torch.mul(out["cl"].reshape(1), float(n), out=self._wacc[4:5])
            if "kd" in out:
                torch.mul(out["kd"].reshape(1), float(n), out=self._wacc[5:6])
        else:
            self._wacc[:2].add_(sc[:2], alpha=float(n))
            self._wacc[2:3].add_(out["kl"].reshape(1), alpha=float(n))
            if "ul" in out:
                self._wacc[3:4].add_(out["ul"].reshape(1), alpha=float(n))
            if "cl" in out:
                self._wacc[4:5].add_(out["cl"].reshape(1), alpha=float(n))
            if "kd" in out:
                self._wacc[5:6].add_(out["kd"].reshape(1), alpha=float(n))

    def _close_begin(self, red, rows):
        """The closing call's part BEFORE its backward: the window's row count onto the device and into the exchange.  False when
        there is nothing to step on (no rows and no other rank)."""
        if rows == 0 and (red is None or red.world == 1):
            return False
        if self._count is None:
            self._count = torch.zeros(1, device=self.eng.dev, dtype=torch.float32)
        self._count.fill_(float(rows))              # asynchronous fill; the value is known on the host
        if red is not None:
            red.start_count(self._count)            # SUM over ranks, in place, asynchronous
        if rows == 0:
            # (a window without rows ran no backward: everything must be zero for the exchange)
            self.eng.zero_grad(None)
        return True

    def _close_end(self, red):
        """Exchange, clip + AdamW, the average, schedule: once per window.  With ema_decay the order is: the average's lazy first
        copy of the master (so that it starts from the weights BEFORE the first optimizer step), the AdamW step, then
        ema += (1 - decay_t) (master - ema) with decay_t computed here in double and the kernel reading the same row count as AdamW."""
        eng = self.eng
        if self.ema_decay is not None:
            eng.ema_init()
        if red is not None:
            if self.measure_finish:     # exposed exchange time: how long the compute stream sits in finish() (bench.py --gpus N)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                red.finish(eng.grad)
                e1.record()
                self.finish_events.append((e0, e1))
            else:
                red.finish(eng.grad)
        eng.adamw_step(self.current_lr(), self.max_norm, self.betas, self.eps, self.wd, count=self._count, groups=self.groups)
        if self.ema_decay is not None:
            t = self.ema_updates
            decay = min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay
            eng.ema_update(1.0 - decay, count=self._count)
            self.ema_updates = t + 1
        self.sched_step += 1
        rows = self._rows
        if rows == 0:
            self.window = {"loss": None, "lm_loss": None, "kl": None, "rows": 0}
            if self.ul_weight > 0.0:
                self.window["ul"] = None
            if self.cl_weight > 0.0:
                self.window["cl"] = None
            if self.distill_weight > 0.0:
                self.window["kd"] = None
        elif self.accumulation_steps == 1:
            self.window = dict(self._wacc, rows=rows)
        else:
            w = self._wacc / float(rows)
            self.window = {"loss": w[0], "lm_loss": w[1], "kl": w[2], "rows": rows}
            if self.ul_weight > 0.0:
                self.window["ul"] = w[3]
            if self.cl_weight > 0.0:
                self.window["cl"] = w[4]
            if self.distill_weight > 0.0:
                self.window["kd"] = w[5]
        self._end_window()

    def _end_window(self):
        self._micro = self._rows = 0
        self._bwd_ran = False

    # ---- the distillation teacher
    @torch.no_grad()
    def _teacher_pass(self, batch, stage):
        """The teacher's side of a micro-step, on the rows the student sees: at distill_scale != 1 its forward on the batch without
        images and texts (eval mode) and the loss, whose logits and row lse go into buffers of the teacher engine's own (as in
        evaluate_guided_batch); then its conditional forward and loss, whose logits and lse stay where they are -- the teacher runs
        nothing else until the next call.  Returns (cond, lse_c, uncond or None, lse_u or None) for Engine.distill_loss."""
        teng = self.teng
        ulog = ulse = None
        if self.distill_scale != 1.0:
            teng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32, exp_drop=NO_EXPERIENCE)
            teng.loss(batch["rating"], stage)
            a = teng.act
            ulog = teng.buf("distill_uncond_logits", tuple(a["logits"].shape), a["logits"].dtype)
            ulse = teng.buf("distill_uncond_lse", (a["M"],), torch.float32)
            ulog.copy_(a["logits"])
            ulse.copy_(a["lse_rows"])
        teng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32)
        teng.loss(batch["rating"], stage)
        return teng.act["logits"], teng.act["lse_rows"], ulog, ulse

    # ---- evaluation (train.py:241-268)
    @torch.no_grad()
    def _eval_rows(self, batch, stage, filter_rows):
        """The stage's row filter of the evaluation passes; None when it leaves no row."""
        if filter_rows and stage in (1, 2):
            idx = curriculum_filter(batch["rating_host"] if "rating_host" in batch else batch["rating"], stage)
            batch = {k: v[idx.to(v.device, non_blocking=True)] for k, v in batch.items() if k != "rating_host"}
        elif "rating_host" in batch:
            batch = {k: v for k, v in batch.items() if k != "rating_host"}
        return None if int(batch["rating"].shape[0]) == 0 else batch

    @torch.no_grad()
    def evaluate_guided_batch(self, batch, scales, negative_batch=None, stage=3, filter_rows=True):
        """The guided validation loss of one batch: the cross-entropy of the held-out lyric under softmax(lu + s (lc - lu)), the
        distribution generate_samples(guidance_scale=s) and GuidedDecoder draw from, for up to eight scales at once (each goes
        through constraints.check_guidance).  The stage's row filter as in evaluate_batch; the negative forward -- negative_batch
        (rows as the batch's; an input it does not name is the batch's own, as in GuidedDecoder.begin), or by default the batch
        itself without its images and texts -- and its loss, whose logits and row lse are copied into buffers of their own (one more
        [M, Vpad] matrix in the logits' storage type); the conditional forward and its loss; mmtg_guided_loss over both.  Returns
        device values, no host sync: {'ce': [K], 'ce_cond': the plain mean of the conditional sample_ce, 'ce_uncond': the negative's,
        'rows': the row count}, or None when the filter leaves no row."""
        scales = _check_scales(scales)
        eng = self.eng
        if negative_batch is not None:
            negative_batch = dict(batch, **negative_batch)
            if int(negative_batch["targets"].shape[0]) != int(batch["targets"].shape[0]):
                raise ValueError("negative_batch: one row per row of the batch")
            if filter_rows and stage in (1, 2):         # the batch's selection, applied to both
                for k in ("rating", "rating_host"):
                    if k in batch:
                        negative_batch[k] = batch[k]
            negative_batch = self._eval_rows(negative_batch, stage, filter_rows)
        batch = self._eval_rows(batch, stage, filter_rows)
        if batch is None:
            return None
        n = int(batch["rating"].shape[0])
        if negative_batch is None:
            eng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32, exp_drop=NO_EXPERIENCE)
        else:
            eng.forward(negative_batch, train_flag=True, training=False, logits_f32=_LOGITS_F32)
        eng.loss(batch["rating"], stage)
        a = eng.act
        # (buffers of their own: the second forward overwrites the engine's logits, row lse and sample_ce)
        ulog = eng.buf("guided_uncond_logits", tuple(a["logits"].shape), a["logits"].dtype)
        ulse = eng.buf("guided_uncond_lse", (a["M"],), torch.float32)
        ulog.copy_(a["logits"])
        ulse.copy_(a["lse_rows"])
        ce_uncond = a["sample_ce"].mean()
        eng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32)
        eng.loss(batch["rating"], stage)
        ce_cond = eng.act["sample_ce"].mean()
        ce = eng.guided_loss(scales, ulog, ulse).clone()        # (the engine's buffer is the next call's as well)
        return {"ce": ce, "ce_cond": ce_cond, "ce_uncond": ce_uncond, "rows": n}

    def evaluate_guided(self, valid_batches, scales, stage=3, negative_batches=None, averaged=False):
        """evaluate_guided_batch over an iterable of validation batches (negative_batches: None or an iterable alongside it): the
        ROW-weighted means over all batches, summed on the device with one host read at the end, so that a scale can be chosen on
        validation data.  Returns {'scales': [...], 'ce': [...], 'ce_cond': x, 'ce_uncond': y, 'rows': n}; the model is in eval mode
        during the pass and gets its previous mode back afterwards.  averaged=True runs the pass inside averaged_weights()."""
        if averaged:
            with self.averaged_weights():
                return self.evaluate_guided(valid_batches, scales, stage, negative_batches)
        scales = _check_scales(scales)
        was_training = self.model.training
        self.model.eval()
        acc, rows = None, 0
        negs = iter(negative_batches) if negative_batches is not None else None
        try:
            for batch in valid_batches:
                out = self.evaluate_guided_batch(batch, scales, None if negs is None else next(negs), stage)
                if out is None:
                    continue
                v = torch.cat([out["ce"], out["ce_cond"].reshape(1), out["ce_uncond"].reshape(1)]) * float(out["rows"])
                acc = v if acc is None else acc + v
                rows += out["rows"]
        finally:
            self.model.train(was_training)
        K = len(scales)
        if rows == 0:
            return {"scales": [float(s) for s in scales], "ce": [0.0] * K, "ce_cond": 0.0, "ce_uncond": 0.0, "rows": 0}
        v = (acc / float(rows)).tolist()
        return {"scales": [float(s) for s in scales], "ce": v[:K], "ce_cond": v[K], "ce_uncond": v[K + 1], "rows": rows}

    @torch.no_grad()
    def evaluate_modality_guided_batch(self, batch, scales, stage=3, filter_rows=True):
        """The per-modality guided validation loss of one batch: the cross-entropy of the held-out lyric under
        lc + sum_k (s_k - 1) (lc - l_k), the distribution generate_samples(guidance_scale=, image_guidance_scale=,
        text_guidance_scale=) and ModalityGuidedDecoder draw from, for up to eight triples (guidance_scale, image_guidance_scale,
        text_guidance_scale) at once (each goes through constraints.check_modality_guidance).  A branch runs if any triple's scale
        for it differs from 1, in the decoder's order u, i, t; its negative is the batch itself without its images and texts, without
        its images or without its texts (exp_drop (1, 0, 0), (0, 1, 0), (0, 0, 1): what generate.without_experience / without_images
        / without_texts feed the decoders).  Each negative's forward and loss run first, and its logits and row lse are copied
        into engine buffers of its own, guided_neg{k}_logits and guided_neg{k}_lse: up to three more [M, Vpad] matrices in the
        logits' storage type, 402 MB each at 64 x 236 in bf16.  The conditional forward and its loss run last, so its logits stay in
        place; then one mmtg_guided_loss_multi launch covers all triples (a triple's scale for a running branch may be 1).  When no
        branch runs -- every triple is (1, 1, 1) -- nothing is launched and every ce is ce_cond.  Returns device values, no host
        sync: {'ce': [G], 'ce_cond': the plain mean of the conditional sample_ce, 'ce_negatives': {'u' / 'i' / 't': the running
        branches' own}, 'rows': the row count}, or None when the filter leaves no row."""
        from .constraints import GUIDANCE_BRANCHES
        scales = _check_scale_triples(scales)
        eng = self.eng
        batch = self._eval_rows(batch, stage, filter_rows)
        if batch is None:
            return None
        n = int(batch["rating"].shape[0])
        running = [j for j in range(3) if any(t[j] != 1.0 for t in scales)]
        neg_logits, neg_lses, ce_neg = [], [], {}
        for k, j in enumerate(running, 1):
            eng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32, exp_drop=tuple(float(i == j) for i in range(3)))
            eng.loss(batch["rating"], stage)
            a = eng.act
            # (buffers of their own: the next forward overwrites the engine's logits, row lse and sample_ce)
            nlog = eng.buf("guided_neg%d_logits" % k, tuple(a["logits"].shape), a["logits"].dtype)
            nlse = eng.buf("guided_neg%d_lse" % k, (a["M"],), torch.float32)
            nlog.copy_(a["logits"])
            nlse.copy_(a["lse_rows"])
            neg_logits.append(nlog)
            neg_lses.append(nlse)
            ce_neg[GUIDANCE_BRANCHES[j]] = a["sample_ce"].mean()
        eng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32)
        eng.loss(batch["rating"], stage)
        ce_cond = eng.act["sample_ce"].mean()
        if running:
            ce = eng.guided_loss_multi([tuple(t[j] for j in running) for t in scales], neg_logits, neg_lses).clone()
        else:
            ce = ce_cond.reshape(1).repeat(len(scales))
        return {"ce": ce, "ce_cond": ce_cond, "ce_negatives": ce_neg, "rows": n}

    def evaluate_modality_guided(self, valid_batches, scales, stage=3, averaged=False):
        """evaluate_modality_guided_batch over an iterable of validation batches: the ROW-weighted means over all batches, summed on
        the device with one host read at the end, so that the image and the text scale can be chosen on validation data
        (best_scale).  Returns {'scales': [(s, s_img, s_txt), ...], 'ce': [...], 'ce_cond': x, 'ce_negatives': {'u' / 'i' / 't': y},
        'rows': n}; the model is in eval mode during the pass and gets its previous mode back afterwards.  averaged=True runs the
        pass inside averaged_weights()."""
        if averaged:
            with self.averaged_weights():
                return self.evaluate_modality_guided(valid_batches, scales, stage)
        scales = _check_scale_triples(scales)
        was_training = self.model.training
        self.model.eval()
        acc, rows, names = None, 0, []
        try:
            for batch in valid_batches:
                out = self.evaluate_modality_guided_batch(batch, scales, stage)
                if out is None:
                    continue
                names = list(out["ce_negatives"])
                v = torch.cat([out["ce"], out["ce_cond"].reshape(1)] + [out["ce_negatives"][k].reshape(1) for k in names]) * float(out["rows"])
                acc = v if acc is None else acc + v
                rows += out["rows"]
        finally:
            self.model.train(was_training)
        G = len(scales)
        if rows == 0:
            from .constraints import GUIDANCE_BRANCHES
            names = [GUIDANCE_BRANCHES[j] for j in range(3) if any(t[j] != 1.0 for t in scales)]
            return {"scales": scales, "ce": [0.0] * G, "ce_cond": 0.0, "ce_negatives": {k: 0.0 for k in names}, "rows": 0}
        v = (acc / float(rows)).tolist()
        return {"scales": scales, "ce": v[:G], "ce_cond": v[G], "ce_negatives": dict(zip(names, v[G + 1:])), "rows": rows}

    @torch.no_grad()
    def evaluate_batch(self, batch, stage=3, filter_rows=True, without_experience=False):
        """Forward + MyLoss (+ KL) of one validation batch, no update: the stage's row filter, the engine's forward in eval mode (no
        dropout) with compute-dtype logits -- no fp32 [B, T, V] tensor, no autograd boundary -- and the loss kernels.  Returns the
        DEVICE scalars {'loss': MyLoss mean, 'kl': kl, 'total': loss + alpha * kl} (no host sync), or None when the filter leaves
        no rows (train.py:252-253 `continue`s).  With ul_weight > 0 also 'ul', the unweighted unlikelihood term of the batch, with cl_weight > 0 also 'cl', with
        distill_weight > 0 also 'kd' (against the teacher's distribution for the batch as given, also under without_experience); 'total'
        stays the reference's validation loss.  without_experience=True runs the forward on the batch without its images and
        texts (generate.without_experience): the validation loss of the branch guidance subtracts."""
        eng = self.eng
        batch = self._eval_rows(batch, stage, filter_rows)
        if batch is None:
            return None
        if self.distill_weight > 0.0:
            teacher = self._teacher_pass(batch, stage)
        if without_experience:
            eng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32, exp_drop=NO_EXPERIENCE)
        else:
            eng.forward(batch, train_flag=True, training=False, logits_f32=_LOGITS_F32)
        sc = eng.loss(batch["rating"], stage)
        loss, kl = sc[0], eng.act["kl"][0]
        out = {"loss": loss, "kl": kl, "total": loss + self.alpha * kl}
        if self.ul_weight > 0.0:
            out["ul"] = eng.ul_loss()[0]
        if self.cl_weight > 0.0:
            out["cl"] = eng.cl_loss(self.cl_margin)[0]
        if self.distill_weight > 0.0:
            out["kd"] = eng.distill_loss(*teacher, scale=self.distill_scale)[0]
        return out

    @torch.no_grad()
    def evaluate(self, valid_batches, stage=3, averaged=False, without_experience=False):
        """The reference's evaluate() (train.py:241-268) over an iterable of validation batches: per batch
        total = MyLoss.mean() + alpha * kl.mean(), summed -- on the device, one host read at the end -- and divided by the NUMBER OF
        BATCHES (filtered-out ones included, as `valid_loss /= len(valid_dataset)` does).  Returns (valid_loss, kldiv_loss) floats;
        the model is in eval mode during the pass (train.py:242) and gets its previous mode back afterwards.
        averaged=True runs the pass inside averaged_weights(); without_experience=True as in evaluate_batch."""
        if averaged:
            with self.averaged_weights():
                return self.evaluate(valid_batches, stage, without_experience=without_experience)
        was_training = self.model.training
        self.model.eval()
        acc = torch.zeros(2, device=self.eng.dev, dtype=torch.float32)
        n = 0
        try:
            for batch in valid_batches:
                n += 1
                out = self.evaluate_batch(batch, stage, without_experience=True) if without_experience else self.evaluate_batch(batch, stage)
                if out is None:
                    continue
                acc[0] += out["total"]
                acc[1] += self.alpha * out["kl"]
        finally:
            self.model.train(was_training)
        if n == 0:
            return 0.0, 0.0
        v = (acc / n).tolist()
        return v[0], v[1]

    # ---- the averaged weights
    def _refuse_averaged(self, what):
        if self._averaged:
            raise RuntimeError("%s inside averaged_weights(): the masters hold the average until the context exits" % what)

    def _require_average(self, what):
        if self.ema_decay is None:
            raise RuntimeError("%s: this trainer keeps no average (ema_decay=None)" % what)
        if self.eng.ema is None:
            raise RuntimeError("%s: there is no average yet (no optimizer step has been taken)" % what)

    @contextlib.contextmanager
    def averaged_weights(self):
        """Context in which the model computes with the averaged weights: master and average are exchanged in place on entry and
        exchanged back on exit (also when the body raises), each time invalidating the derived copies, so evaluate*, the model's
        forward and every decoder or generator built on this model read the average inside and the last iterate after.  step(),
        flush(), state_dict(), load_state_dict() and a nested entry raise inside; entering inside an open accumulation window is
        fine, gradients are not touched."""
        self._refuse_averaged("averaged_weights()")
        self._require_average("averaged_weights()")
        self.eng.swap_ema()
        self._averaged = True
        try:
            yield self
        finally:
            self.eng.swap_ema()
            self._averaged = False

    def ema_state_dict(self):
        """The averaged model as CPU tensors with the keys, shapes and dtypes of model.state_dict(): every key of the flat buffer
        (the tied lm_head included) from the average, anything else from the model.  Loads into another MMTG."""
        self._require_average("ema_state_dict()")
        eng = self.eng
        flat = (eng.master if self._averaged else eng.ema).detach().cpu()
        out = {}
        for k, v in self.model.state_dict().items():
            key = "decoder.gpt2.transformer.wte.weight" if k == "decoder.gpt2.lm_head.weight" else k
            if key in eng.layout.entries:
                out[k] = eng.layout.view(flat, key).clone()
            else:
                out[k] = v.detach().cpu().clone()
        return out

    def finish_wait_ms(self):
        """Mean time per step the compute stream waited in the reducer's finish() -- the part of the gradient exchange the
        backward did NOT hide -- over the steps taken with ``measure_finish`` on (synchronises; clears the record)."""
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.finish_events]
        self.finish_events = []
        return sum(ms) / len(ms) if ms else None

    def grad_norm(self):
        """Global gradient norm of the last step as clip_grad_norm_ saw it (device scalar): the flat buffer holds row
        sums, so sqrt(sum g^2) / global row count."""
        return torch.sqrt(self.eng.normsq[0]) / self._count[0]

    def group_grad_norms(self):
        """Per-group gradient norms of the last step (device vector, one entry per group, the implicit group last; 0 for a frozen
        group): sqrt(sum over the group's tensors of g^2) / global row count.  With frozen groups grad_norm() is the norm of the
        trainable tensors, as clip_grad_norm_ sees it when frozen parameters have no gradient."""
        if self.groups is None:
            raise RuntimeError("group_grad_norms: this trainer has no param_groups")
        return torch.sqrt(self.eng.group_normsq[:self.groups.ngroups]) / self._count[0]

    def describe_groups(self):
        """One dict per group, the implicit group of unmatched keys last: the spec as given (None for the implicit group), the
        resolved lr_scale / weight_decay / frozen, and how many tensors and parameters the group holds."""
        if self.group_plan is None:
            return []
        return [{"spec": copy.deepcopy(g["spec"]), "lr_scale": g["lr_scale"], "weight_decay": g["weight_decay"], "frozen": g["frozen"],
                 "tensors": len(g["keys"]), "parameters": g["parameters"]} for g in self.group_plan.groups]


def save_checkpoint(path, model, trainer=None, args=None, model_cfgs=None, reference_compatible=False, averaged=False):
    """The reference's checkpoint dict ``{'model', 'args', 'model_cfgs'}`` (train.py:212) plus, when a trainer is
    given, ``'trainer'`` for resuming.

    reference_compatible=True writes the state dict exactly as the reference's own run would have: keys carry the
    ``module.`` prefix of its nn.DataParallel wrapper (train.py:113,212) and every GPT-2 block has the persistent
    ``attn.bias`` / ``attn.masked_bias`` buffers of transformers 4.12.3, so the reference's strict
    ``load_state_dict`` into its DataParallel-wrapped model (generate.py:191-192) accepts the file.  The default
    writes ``model.state_dict()`` (what ``load_checkpoint`` and any unwrapped consumer read).

    averaged=True writes the ``'model'`` entry from the trainer's averaged weights (``trainer.ema_state_dict()``), in either key
    style: a file for evaluation and generation.  ``'trainer'`` still holds the raw trainer state -- moments, counters, the
    average -- but the last iterate's parameters are in no entry: resume from a file written without the flag.  It raises when
    there is no trainer or the trainer has no average."""
    if averaged:
        if trainer is None:
            raise RuntimeError("save_checkpoint(averaged=True) needs the trainer that keeps the average")
        avg = trainer.ema_state_dict()
    if reference_compatible:
        sd = {"module." + k: v for k, v in model.legacy_state_dict().items()}
        if averaged:
            sd.update(("module." + k, v) for k, v in avg.items())
    else:
        sd = avg if averaged else model.state_dict()
    ckpt = {"model": {k: v.detach().cpu() for k, v in sd.items()}, "args": args, "model_cfgs": model_cfgs}
    if trainer is not None:
        ckpt["trainer"] = trainer.state_dict()
    torch.save(ckpt, path)


def load_checkpoint(path, model, trainer=None):
    """Loads a checkpoint written by ``save_checkpoint`` or by the reference's train.py ('module.' prefixes and
    transformers-4.12.3 buffers accepted).  Returns the checkpoint dict."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(ckpt["model"] if "model" in ckpt else ckpt)
    if trainer is not None and ckpt.get("trainer") is not None:
        trainer.load_state_dict(ckpt["trainer"])
    return ckpt
