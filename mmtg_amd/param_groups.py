"""Optimizer parameter groups on the flat parameter layout (host side, no GPU needed).

Specs are dicts as torch's optimizers take them, with fnmatch patterns on the state-dict keys in place of tensors:

    {"params": pattern | [patterns], "lr_scale": 1.0, "weight_decay": None, "frozen": False}

The first spec that matches a key wins; keys matched by no spec form an implicit last group (lr_scale 1, the trainer's
weight_decay).  ``[{"params": ["*bias*", "*ln_*"], "weight_decay": 0.0}]`` is the ``no_decay`` list of the transformers fine-tuning
scripts, ``[{"params": "decoder.gpt2.*", "frozen": True}]`` freezes the pretrained decoder.

The plan's ``segments`` are what the grouped step kernels (mmtg_sumsq_groups, mmtg_adamw_groups) walk: exact key ranges of the flat
buffer, so the alignment gaps between packs and the tail pad of the embedding never belong to a segment.
"""
from __future__ import annotations

import copy
import fnmatch
import math

import numpy as np

MAX_GROUPS = 16          # MMTG_MAX_PARAM_GROUPS
MAX_SEGMENTS = 1024      # MMTG_MAX_PARAM_SEGS
_SPEC_KEYS = ("params", "lr_scale", "weight_decay", "frozen")


class ParamGroupPlan:
    """segments: int64 [S, 3] of (begin, end, group), sorted and disjoint; groups: one dict per group (the implicit one last) with
    'spec' (the user's dict, None for the implicit group), 'lr_scale', 'weight_decay', 'frozen', 'keys', 'parameters'; specs: a
    copy of the list the plan was built from; total: the layout's element count."""

    def __init__(self, segments, groups, specs, total):
        self.segments, self.groups, self.specs, self.total = segments, groups, specs, total

    def group_of(self, key):
        for i, g in enumerate(self.groups):
            if key in g["keys"]:
                return i
        raise KeyError(key)


def _number(what, i, x):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(x) or x < 0:
        raise ValueError("param_groups[%d]: %s = %r must be a finite number >= 0" % (i, what, x))
    return float(x)


def build_param_groups(layout, specs, weight_decay=0.0):
    """The group table of `specs` on `layout` (engine.ParamLayout).  Raises ValueError naming the offender for a pattern that
    matches no key, more than 16 groups (the implicit one included), a negative or non-finite lr_scale / weight_decay, an
    unknown dict key."""
    default_wd = _number("the trainer's weight_decay", -1, weight_decay)
    specs = [] if specs is None else list(specs)
    if len(specs) + 1 > MAX_GROUPS:
        raise ValueError("param_groups: %d groups with the implicit last one (at most %d)" % (len(specs) + 1, MAX_GROUPS))
    groups = []
    for i, spec in enumerate(specs):
        if not isinstance(spec, dict):
            raise ValueError("param_groups[%d]: %r is not a dict" % (i, spec))
        for k in spec:
            if k not in _SPEC_KEYS:
                raise ValueError("param_groups[%d]: unknown key %r (known: %s)" % (i, k, ", ".join(_SPEC_KEYS)))
        if "params" not in spec:
            raise ValueError("param_groups[%d]: no 'params'" % i)
        pats = [spec["params"]] if isinstance(spec["params"], str) else list(spec["params"])
        for pat in pats:
            if not isinstance(pat, str):
                raise ValueError("param_groups[%d]: pattern %r is not a string" % (i, pat))
            if not any(fnmatch.fnmatchcase(k, pat) for k in layout.keys):
                raise ValueError("param_groups[%d]: pattern %r matches no parameter" % (i, pat))
        wd = spec.get("weight_decay")
        frozen = spec.get("frozen", False)
        if not isinstance(frozen, (bool, np.bool_)):
            raise ValueError("param_groups[%d]: frozen = %r must be a bool" % (i, frozen))
        groups.append({"spec": copy.deepcopy(spec), "patterns": pats, "lr_scale": _number("lr_scale", i, spec.get("lr_scale", 1.0)),
                       "weight_decay": default_wd if wd is None else _number("weight_decay", i, wd), "frozen": bool(frozen),
                       "keys": [], "parameters": 0})
    groups.append({"spec": None, "patterns": [], "lr_scale": 1.0, "weight_decay": default_wd, "frozen": False, "keys": [], "parameters": 0})
    segs = []
    for key in sorted(layout.keys, key=lambda k: layout.entries[k][0]):
        off, _, n = layout.entries[key]
        gi = next((i for i, g in enumerate(groups) if any(fnmatch.fnmatchcase(key, p) for p in g["patterns"])), len(groups) - 1)
        groups[gi]["keys"].append(key)
        groups[gi]["parameters"] += n
        if n == 0:
            continue
        if segs and segs[-1][1] == off and segs[-1][2] == gi:
            segs[-1][1] = off + n                       # neighbours of one group that touch: one segment
        else:
            segs.append([off, off + n, gi])
    if len(segs) > MAX_SEGMENTS:
        raise ValueError("param_groups: %d segments (at most %d); fewer, coarser groups merge more neighbours" % (len(segs), MAX_SEGMENTS))
    return ParamGroupPlan(np.asarray(segs, dtype=np.int64).reshape(-1, 3), groups, copy.deepcopy(specs), int(layout.total))
