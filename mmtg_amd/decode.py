"""Batched greedy generation with a KV cache and a replayed hipGraph per token.

The reference decodes one sample at a time and re-runs the whole model on the growing
prefix for every token (src/generate.py:117-145, O(L^2), ~198 full forwards per sample).
Here every row of a batch advances in lock step, one token per step, against per-layer
K/V caches; the step is a fixed launch sequence whose only varying input -- the position --
lives in device memory, so it is captured once into a hipGraph and replayed.

Semantics kept from the reference: forced [#EOS#]/[#START#] cadence every 22 slots,
per-occurrence repetition penalty, temperature, banned ids, sticky PAD, inference-branch
type ids / key mask.  The type-id / mask rule is applied per row (the reference reads row 0
only because it never batches; identical at batch 1).
"""
from __future__ import annotations

import inspect
import os

import numpy as np
import torch

from . import hip
from .constraints import (BANNED, GUIDANCE_OFF, MIROSTAT_OFF, WARP_OFF, KeywordTables, LineTables, _check_constraints, check_contrastive, check_groups, check_guidance, check_keywords, check_lines,  # noqa: F401
                          check_mirostat, check_ngram, check_prefix, check_refrain, check_stochastic, check_warp, chosen_mask, keywords_met, refrain_without_keywords,
                          sequence_scores, stochastic_row_seeds)   # (the host-side checks keep their names here)

_PLACEMENT = {}


def select_forms(with_head, prefix, ngram, lines, templates=False, rhymes=False, groups=False, keywords=False, refrain=False,
                 copies=False):
    """Which selection entries a token step ends in: (form of mmtg_decode_select / _sample or mmtg_decode_beam_candidates, form of
    mmtg_decode_beam_merge), each "" (plain), "_fixed", "_ngram", "_lines", "_tmpl", "_rhyme" or "_refrain".  with_head: the step calls the
    model's head; prefix: the generation has one; ngram: no_repeat_ngram_size; lines: line constraints are given; templates: line
    templates are given (every step that calls the head then ends in "_tmpl"); rhymes: a rhyme scheme is given (every such step
    ends in "_rhyme", with or without templates).  The bans act where logits are read, so
    a step without the head (select with null logits; no candidates launch, merge with null candidates) and every merge only know
    the prefix -- a generation without constraints runs the plain entries throughout.  groups: the beams are in more than one
    group (diverse beam search): the merge of a step with the head is then "_groups" / "_groups_fixed"; a step without the head
    has no candidates to choose among and keeps the merge it always ran.  keywords: the prompts carry keywords (keyword-constrained
    beam search): a step with the head ends in the "_kw" candidates -- one entry over the rhyme form, which serves every rule above
    or none -- and the "_kw" / "_kw_fixed" merge; a step without the head keeps the merge it always ran.  refrain: a refrain scheme is
    given: every step that calls the head ends in "_refrain", whatever other rules there are (the form is the rhyme form plus the
    copy).  copies (GreedyDecoder, with a scheme): the step skipped the head because every row is held by its prefix or copies; it
    ends in "_refrain" with null logits, which writes the copies.  Every other step without the head is what it always was."""
    held = "_fixed" if prefix else ""
    if not with_head:
        return ("_refrain" if refrain and copies else held), held
    if keywords:
        return "_kw", "_kw" + held
    return (("_refrain" if refrain else "_rhyme" if rhymes else "_tmpl" if templates else "_lines" if lines else "_ngram" if ngram else held),
            "_groups" + held if groups else held)


class StepRules:
    """What one generation decided about its token steps: built once, in ``begin``, and not changed afterwards.  Every field's default
    is "off", so ``StepRules()`` is a generation without rules: the plain entries and nothing in the graph key.  What changes from
    step to step (whether the step calls the head, whether it is a copy step) is an argument of the methods; the rows' state
    (uniforms, mirostat_mu, tok_lp, gum) and fixed_end, a view each decoder holds since its construction, stay on the decoder.

    prefix: the generation has one: the steps end in the *_fixed selection entries.  ngram: no_repeat_ngram_size.
    lines: the device tables (lo, hi, sets or None, set_of or None) of line_lengths= / line_end_ids=.  tmpl: the int32 symbol table
    [B, lines, sent - 2] of templates=.  rhyme: (class_of int16 [V], lead int8 [B, lines], distinct) of rhyme_scheme=.  refrain: src
    int8 [B, lines] of refrain_scheme=.  Each of them, when not None, ends every step that calls the head in the selection entries
    of its form (``select_forms``).
    warp: (min_p, typical_p, epsilon_cutoff, eta_cutoff); any of them on ends every step that calls the head in
    mmtg_decode_sample_warp.  warp_src: an all -1 src table, what that entry takes without a refrain scheme.
    mirostat: (tau, eta); tau > 0 ends every step that calls the head in mmtg_decode_sample_mirostat.
    return_logprobs: every step that calls the head ends in one more launch, mmtg_decode_logprob.
    groups, diversity_penalty: the beam groups of a diverse beam search.  kw: (phrases int32 [prompts, 8, 4], lens int8 [prompts, 8],
    K, the longest phrase) of keywords=; not None ends every step that calls the head in the *_kw entries."""
    __slots__ = ("prefix", "ngram", "lines", "tmpl", "rhyme", "refrain", "warp", "warp_src", "mirostat", "return_logprobs", "groups",
                 "diversity_penalty", "kw")

    def __init__(self, prefix=False, ngram=0, lines=None, tmpl=None, rhyme=None, refrain=None, warp=WARP_OFF, warp_src=None,
                 mirostat=MIROSTAT_OFF, return_logprobs=False, groups=1, diversity_penalty=0.0, kw=None):
        self.prefix, self.ngram, self.lines, self.tmpl, self.rhyme, self.refrain = prefix, ngram, lines, tmpl, rhyme, refrain
        self.warp, self.warp_src, self.mirostat, self.return_logprobs = warp, warp_src, mirostat, return_logprobs
        self.groups, self.diversity_penalty, self.kw = groups, diversity_penalty, kw

    def rows(self, a, z):
        """The record of rows a .. z - 1 of the batch (a lane's): views of the per-row tables, the shared ones (sets, class_of) as
        they are."""
        cut = lambda t: None if t is None else t[a:z]                           # noqa: E731
        lines, rhyme = self.lines, self.rhyme
        return StepRules(self.prefix, self.ngram, None if lines is None else (lines[0][a:z], lines[1][a:z], lines[2], cut(lines[3])),
                         cut(self.tmpl), None if rhyme is None else (rhyme[0], rhyme[1][a:z], rhyme[2]), cut(self.refrain), self.warp,
                         cut(self.warp_src), self.mirostat, self.return_logprobs, self.groups, self.diversity_penalty, self.kw)

    def forms(self, with_head, copies=False):
        """select_forms' answer for a step of this generation, and whether mmtg_decode_logprob follows it: (selection form, merge
        form, logprob).  copies: the step skipped the head because every row copies or is held."""
        return select_forms(with_head, self.prefix, self.ngram, self.lines is not None, templates=self.tmpl is not None,
                            rhymes=self.rhyme is not None, groups=self.groups > 1, keywords=self.kw is not None,
                            refrain=self.refrain is not None, copies=copies) + (bool(with_head and self.return_logprobs),)

    def _rhyme_key(self):
        """What a captured launch of the rhyme form holds by value: end sets or bounds only, the template table or none, a scheme's
        distinct flag (the "_kw" candidates run the form with line tables but possibly without a scheme: "lines" then)."""
        return (("lines" if self.rhyme is None else "rhyme", "sets" if self.lines[2] is not None else "bounds")
                + (("tmpl",) if self.tmpl is not None else ()) + (("distinct",) if self.rhyme is not None and self.rhyme[2] else ()))

    def _refrain_key(self):
        """What a captured launch of the refrain form holds by value: which of the rhyme form's tables are there at all (line tables
        with end sets or bounds only, the template table, a rhyme scheme and its distinct flag)."""
        return (("refrain",) + (("sets" if self.lines[2] is not None else "bounds",) if self.lines is not None else ())
                + (("tmpl",) if self.tmpl is not None else ())
                + ((("rhyme",) + (("distinct",) if self.rhyme[2] else ())) if self.rhyme is not None else ()))

    def src_key(self):
        """The same for an entry over the refrain form that always takes a src (the warp, Mirostat and Gumbel entries): the refrain
        form's tables, and whether src is a scheme's or the all -1 one."""
        return self._refrain_key() + (("src",) if self.refrain is not None else ())

    def key(self, with_head, copies=False):
        """What a decoder's graph key holds behind (with_head, parity, params): the rules as far as select_forms lets them reach
        this step (a step without the head runs the launches it always ran), each by what the captured launches hold by value."""
        form, merge, logprob = self.forms(with_head, copies)
        key = (("prefix",) if self.prefix else ()) + (("ngram", self.ngram) if self.ngram else ())
        if form in ("_lines", "_tmpl"):
            key += (form[1:], "sets" if self.lines[2] is not None else "bounds")
        if form == "_rhyme":
            key += self._rhyme_key()
        if form == "_refrain":
            key += self._refrain_key()
        mirostat = with_head and self.mirostat[0] > 0.0
        if with_head and (mirostat or self.warp != WARP_OFF):       # (the four cuts by value, whichever of the two entries runs)
            key += (("warp",) + self.warp,) + self.src_key()
        if mirostat:                                                # (tau and eta by value; the state's address never changes)
            key += (("mirostat",) + self.mirostat,)
        if logprob:
            key += ("logprob",)
        if merge.startswith("_groups"):     # (the grouped merge holds both by value)
            key += (("groups", self.groups, float(self.diversity_penalty)),)
        if form == "_kw":                   # (K and the phrase bound by value; then what the rhyme form under them holds by value)
            key += (("kw", self.kw[2]), ("cap", self.kw[3]))
            if self.lines is not None:
                key += self._rhyme_key()
        return key

    def tail(self, fixed_end, entry="form", spare=None):
        """The trailing keyword arguments of the hip selection and candidate calls; fixed_end: the decoder's own view, passed on with
        a prefix only.  entry "form": an entry select_forms names -- it takes the refrain table as refrain= (and reads it in the
        "_refrain" form only).  "src": an entry over the refrain form that always takes a src -- the scheme's table, or without a
        scheme an all -1 one: `spare` if given, else warp_src.  "kw": the keyword candidates, which run the rhyme form -- line tables
        without a scheme get `spare`, a rhyme triple whose lead table names no leader."""
        kw = {"fixed_end": fixed_end if self.prefix else None, "ngram": self.ngram, "tables": self.lines, "tmpl": self.tmpl,
              "rhyme": self.rhyme}
        if entry == "form":
            kw["refrain"] = self.refrain
        elif entry == "src":
            kw["src"] = self.refrain if self.refrain is not None else self.warp_src if spare is None else spare
        elif self.rhyme is None and self.lines is not None:
            kw["rhyme"] = spare
        return kw


def _keywords_need_beams(keywords):
    if keywords is not None:
        raise ValueError("keywords= needs beams: a lyric that contains given words is found by a search over several hypotheses "
                         "(BeamDecoder / generate_beams), not by greedy decoding or sampling")


def _fill(buf, src, fill, axis):
    """The host array src into the device buffer buf (allocated once: captured graphs hold its address), which is longer along
    `axis`; the rest of buf becomes `fill`."""
    full = np.full(tuple(buf.shape), fill, src.dtype)
    full[(slice(None),) * axis + (slice(0, src.shape[axis]),)] = src
    return buf.copy_(torch.from_numpy(full))


def _placement_ok(dev):
    """True when a 256-workgroup, one-per-CU launch puts workgroups b and b + 8 k on one XCD, 32 per XCD (census kernel, once per
    device and process): what the plain hand-off of mmtg_decode_mlp relies on (the launch itself re-checks every group)."""
    key = str(dev)
    if key not in _PLACEMENT:
        c = hip.decode_mlp_census(dev)
        _PLACEMENT[key] = bool(((c == 32).sum(1) == 1).all() and ((c == 32).sum(0) == 1).all() and int(c.sum()) == 256)
    return _PLACEMENT[key]


class GreedyDecoder:
    _skips_copies = True            # a step whose every row copies (refrain_scheme=) or is held skips the head
    _prefill_prompt_only = False    # with a prefix, prefill the prompt alone (ContrastiveDecoder: every lyric column through a step)

    def __init__(self, model, max_batch, max_len=None, use_graph=True, lanes=None, _parent=None, _lane=0):
        self.model = model
        self.eng = model.engine()
        sh = self.eng.sh
        self.B = max_batch
        self.max_len = sh.max_seq_length if max_len is None else max_len      # lyric positions incl. the first [#START#]
        self.Tmax = sh.P + self.max_len + 1
        if self.Tmax > sh.NP:
            raise ValueError("prompt + max_len exceeds n_positions")
        self.use_graph = use_graph
        dev, tdt = self.eng.dev, self.eng.tdt
        B, D, H, E = self.B, sh.D, sh.H, sh.E
        # bf16: deterministic split-K products (K slices per product: c_attn, attn c_proj, c_fc, mlp c_proj)
        # fp32 (the parity mode): the same split-K schedule through the fp32 kernel's slab epilogue (128x128 tiles, so more
        # K slices: 6-24 workgroups per product otherwise)
        self.fast = not os.environ.get("MMTG_DECODE_PLAIN")
        bf = self.eng.dtype == hip.BF16
        # Lanes (opt-in, MMTG_DECODE_LANES / lanes=): the rows of a batch never interact, so the batch can be cut into
        # `lanes` row blocks whose launch chains run side by side on their own streams (fork / join inside the captured
        # graph).  Every row goes through the same arithmetic in the same order whatever the lane count, so the ids do
        # not depend on it (tests/test_decode_gpu.py).  Measured at batch 256 (profiles/r02_v5_decode_lanes_ab.txt):
        # 1 lane 758 us per token step, 2 lanes 825, 4 lanes 1452, 8 lanes 2785 -- hipGraph replay on this ROCm runs
        # the branches one after another and adds a cross-stream dependency per fork / join, so the default stays 1.
        if _parent is not None:
            lanes = 1
        elif lanes is None:
            lanes = int(os.environ.get("MMTG_DECODE_LANES", "1")) if (self.fast and B >= 128) else 1
        if lanes < 1 or B % lanes:
            raise ValueError("batch %d does not divide into %d lanes" % (B, lanes))
        self.lanes = lanes
        if _parent is None:
            self.seq = torch.zeros(B, self.Tmax, dtype=torch.long, device=dev)
            # the position lives in a PAIR of slots per lane: the kernels of step k read slot k % 2, the step's last kernel
            # (decode_select) writes k + 1 into the other one -- no separate "advance" launch, two captured graphs per setting
            self.pos_all = torch.zeros(2, lanes, dtype=torch.int32, device=dev)
            # prefixed generation: row b's seq is host-written up to position fixed_end[b] (the *_fixed selection entries)
            self.fixed_end = torch.zeros(B, dtype=torch.int32, device=dev)
            self.keep = torch.zeros(B, self.Tmax, dtype=torch.int32, device=dev)
            self.types = torch.zeros(B, dtype=torch.long, device=dev)
            self.tpw_type = torch.zeros(B, sh.P, dtype=torch.long, device=dev)
            self.tpw_mask = torch.zeros(B, sh.P, dtype=torch.long, device=dev)
            self.c = torch.zeros(B * sh.S, E, dtype=tdt, device=dev)
            self.kc = torch.zeros(sh.L, B, sh.nH, self.Tmax, 64, dtype=tdt, device=dev)
            self.vc = torch.zeros_like(self.kc)
            self.pos_pair = (self.pos_all[0, 0:1], self.pos_all[1, 0:1])
        else:       # a lane: row block [_lane*B, (_lane+1)*B) of the parent's state, private scratch
            lo, hi = _lane * B, (_lane + 1) * B
            self.seq, self.keep, self.types = _parent.seq[lo:hi], _parent.keep[lo:hi], _parent.types[lo:hi]
            self.fixed_end = _parent.fixed_end[lo:hi]
            self.tpw_type, self.tpw_mask = _parent.tpw_type[lo:hi], _parent.tpw_mask[lo:hi]
            self.c = _parent.c[lo * sh.S:hi * sh.S]
            self.kc = [_parent.kc[l, lo:hi] for l in range(sh.L)]
            self.vc = [_parent.vc[l, lo:hi] for l in range(sh.L)]
            self.pos_pair = (_parent.pos_all[0, _lane:_lane + 1], _parent.pos_all[1, _lane:_lane + 1])
        # (K slices of c_attn, attn c_proj, c_fc, mlp c_proj.  Fused step -- no finish launches, the reduction runs in the product's
        #  own tail -- measured at batch 256, us per token step: 2,4,1,4 -> 714-716; 2,3,1,4 -> 715; 2,2,1,4 -> 721; 3,4,1,4 -> 720;
        #  2,4,1,3 -> 726; 2,4,1,8 -> 728; 2,4,1,6 -> 739; 2,6,1,4 -> 746; 2,4,1,2 -> 751; 4,4,1,4 -> 755; profiles/r03_v8_*)
        fused_ok = self.eng.dtype == hip.BF16 and not os.environ.get("MMTG_DECODE_PLAIN") and os.environ.get("MMTG_DECODE_FUSED", "1") != "0"
        # Round 5, the split-precision step (compute_dtype="bf16x3"): the fused step's launch structure on (hi | lo) plane pairs --
        # fp32 residual stream / KV cache / logits, every product three bf16 matrix-core passes (mmtg_decode_gemm_x3).
        # MMTG_DECODE_X3=0 keeps the exact-fp32 kernels (the f32 mode's step) for the A/B.
        self.x3 = (bool(getattr(self.eng, "x3", False)) and self.fast and os.environ.get("MMTG_DECODE_X3", "1") != "0"
                   and D % 64 == 0 and D // 32 <= hip.DG_NP and H % 64 == 0 and E % 64 == 0 and self.eng.layout.Vpad % 4 == 0)
        self.splits = tuple(int(x) for x in os.environ.get(
            "MMTG_DECODE_SPLITS", "2,4,1,8" if self.x3 else ("2,4,1,4" if fused_ok else "2,4,1,8") if bf else "8,12,8,24").split(","))
        # (measured at batch 256, us per token step: 2,3,2,6 -> 1020; 4,6,3,12 -> 1248; 1,1,1,2 -> 1183; unsplit 1264;
        #  with the one-slice c_fc + fused GELU: 2,3,1,8 -> 940, 2,3,1,6 -> 943, 1,3,1,8 -> 963, 2,3,1,12 -> 1003)
        #  round 2, 64x64 tiles (graph-replayed per-product times, profiles/r02_decode_gemm_tiles.log): 2,4,1,8)
        self.children, self.side = [], []
        self.fused = self.mlp = False       # (set below for a decoder that runs the step itself: not the parent of row blocks)
        if lanes > 1:
            self.children = [GreedyDecoder(model, B // lanes, max_len, use_graph=False, _parent=self, _lane=i) for i in range(lanes)]
            self.side = [torch.cuda.Stream(device=dev) for _ in range(lanes - 1)]
        else:
            z = lambda *s: torch.empty(*s, dtype=tdt, device=dev)
            self.x, self.h1 = z(B, E), z(B, H)
            self.h, self.h2 = z(B, D), z(B, D)
            self.a, self.qkv, self.ctx = z(B, D), z(B, 3 * D), z(B, D)
            self.u, self.g = z(B, 4 * D), z(B, 4 * D)
            self.mu = torch.empty(B, dtype=torch.float32, device=dev)
            self.rs = torch.empty(B, dtype=torch.float32, device=dev)
            self.logits = torch.empty(B, self.eng.layout.Vpad, dtype=torch.float32, device=dev)
            if self.fast:
                slab = max(self.splits[0] * 3 * D, self.splits[1] * D, self.splits[2] * 4 * D, self.splits[3] * D)
                self.part = torch.empty(slab * B, dtype=torch.float32, device=dev)
            if self.x3:
                L, Vp = sh.L, self.eng.layout.Vpad
                f32 = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=dev)
                PL = lambda r, c_: hip.Planes.empty(r, c_, dev)
                self.xp, self.h1p = PL(B, E), PL(B, H)
                self.hp, self.h2p = PL(B, D), PL(B, D)
                self.ctxp, self.gp = PL(B, D), PL(B, 4 * D)
                self.fq = [(PL(3 * D, D), f32(3 * D), f32(3 * D)) for _ in range(L)]          # gamma-folded c_attn plane pair, column sums, folded bias
                self.ffc = [(PL(4 * D, D), f32(4 * D), f32(4 * D)) for _ in range(L)]
                self.fh = (PL(Vp, D), f32(Vp), f32(Vp))
                self.st = (torch.zeros(B, hip.DG_NP, 2, dtype=torch.float32, device=dev),
                           torch.zeros(B, hip.DG_NP, 2, dtype=torch.float32, device=dev))
                # K slices of the two projector products (K = 2048 / 512): in-kernel reduction like attn.c_proj
                self.psplits = tuple(int(x) for x in os.environ.get("MMTG_DECODE_X3_PSPLITS", "8,2").split(","))
                rt = -(-B // 64)
                tiles = rt * max(D // 64, H // 64)
                self.rws = f32(tiles * max(self.splits[1], self.splits[3], *self.psplits) * 4096)
                self.rcnt = torch.zeros(tiles * 4, dtype=torch.int32, device=dev)
            # Round 3, fused step (5 graph nodes per block instead of 7): split-K products reduced in the kernel by the last-arriving
            # wave (+ bias + residual + LayerNorm statistics), LayerNorms applied algebraically in the consuming products
            # (mmtg_decode_gemm).  MMTG_DECODE_FUSED=0 keeps the round-2 products + finish launches.
            self.fused = (self.fast and bf and os.environ.get("MMTG_DECODE_FUSED", "1") != "0" and D % 64 == 0 and D // 32 <= hip.DG_NP
                          and self.eng.layout.Vpad % 4 == 0)
            if self.fused:
                L, Vp = sh.L, self.eng.layout.Vpad
                bf = lambda *s_: torch.empty(*s_, dtype=torch.bfloat16, device=dev)
                f32 = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=dev)
                self.fq = [(bf(3 * D, D), f32(3 * D), f32(3 * D)) for _ in range(L)]          # gamma-folded c_attn copy, column sums, folded bias
                self.ffc = [(bf(4 * D, D), f32(4 * D), f32(4 * D)) for _ in range(L)]
                self.fh = (bf(Vp, D), f32(Vp), f32(Vp))
                self.st = (torch.zeros(B, hip.DG_NP, 2, dtype=torch.float32, device=dev),
                           torch.zeros(B, hip.DG_NP, 2, dtype=torch.float32, device=dev))
                tiles = -(-B // 64) * (D // 64)
                self.rws = f32(tiles * max(self.splits[1], self.splits[3]) * 4096)
                self.rcnt = torch.zeros(tiles * 4, dtype=torch.int32, device=dev)
                self.folds_for = None
                # (MMTG_DECODE_EMBED_IN_PROJ=0: projector_layer2 and the embedding add as two launches, the round-3 v8 step)
                self.embed_in_proj = os.environ.get("MMTG_DECODE_EMBED_IN_PROJ", "1") != "0" and H % 8 == 0
                # Round 6: c_fc -> GELU -> mlp.c_proj of a block as ONE launch (mmtg_decode_mlp): the hidden dimension is split over the
                # XCDs, so the GEMM -> GEMM hand-off stays on one L2 and every weight crosses the fabric once; 4 graph nodes per
                # block instead of 5.  Built for n_embd = 768 and up to 256 rows, parity-tested, and OPT-IN (MMTG_DECODE_MLP=1):
                # measured at batch 256 it ties the two launches stand-alone (20.2 against 20.8 us; 17.6 against 19.2 at 128 rows)
                # and loses inside the token step (713-720 against 682-695 us): the boundary it removes costs 1.1-1.7 us
                # (profiles/r06_v2_graph_node_floor_by_launch_shape.txt) + a ~2 us first-tile ramp, the hand-off that replaces it
                # 0.96 us of store acknowledgement + 2.75 us of wait (arrival skew of the 8 producers) + 0.69 us of reload
                # (profiles/r06_v2_decode_mlp_in_step_timeline.txt), and the 8-way cross-XCD reduction has a longer tail than the
                # 4-way one.  MMTG_DECODE_MLP_HANDOFF=plain: through the L2 (checked per launch; slower in the step: its partial-line
                # stores fetch lines); default sc1 (write-through + agent-scope loads: valid under any workgroup placement).
                # Never for the row blocks of a multi-lane decoder: its 256 workgroups must be co-resident, which side-by-side
                # launches on several streams cannot promise.
                self.mlp = _parent is None and D == 768 and B <= 256 and os.environ.get("MMTG_DECODE_MLP") == "1"
                if self.mlp:
                    self.mlp_ws = f32(hip.decode_mlp_ws_floats(B))
                    self.mlp_sync = torch.zeros(hip.decode_mlp_sync_words(), dtype=torch.int64, device=dev)
                    self.mlp_plain = os.environ.get("MMTG_DECODE_MLP_HANDOFF", "sc1") == "plain"
                    self.mlp_trace = None
                    if self.mlp_plain and not _placement_ok(dev):
                        self.mlp_plain = False          # workgroups b and b + 8 k do not share an XCD here: write-through hand-off
        self.pos, self.pos_next = self.pos_pair
        # the prompt in one batched pass (round 5; MMTG_DECODE_PREFILL=0: P token steps, as rounds 1-4 ran it)
        self.prefill = _parent is None and os.environ.get("MMTG_DECODE_PREFILL", "1") != "0"
        self.first_pos = 0
        self.uniforms = None
        self.graphs = {}
        self.params = None
        self.rows = None            # the ancestry table of beam search (BeamDecoder); None: row b attends over its own cache row
        # what the generation decided about its steps (``begin`` builds it once; a lane holds the record of its own rows)
        self.rules = StepRules()
        self.min_fixed = 0          # min over rows of fixed_end (a step below it appends nothing: no head needed)
        # the rules' device tables, all rows, each allocated once by its _upload_*: captured graphs hold the addresses.  _line_buf:
        # (lo, hi, set_of) [B, lines of max_len] and the growing `sets` buffer; _warp_buf: the all -1 src of StepRules.warp_src
        self._line_buf = self._tmpl_buf = self._rhyme_buf = self._refrain_buf = self._warp_buf = None
        # copy_cols (host, bool [1 + length], the parent's): the lyric columns at which every row is held by its prefix or copies
        # under the refrain scheme, so the step skips the head; copy_step: the step being run is one of those (it ends in
        # mmtg_decode_select_refrain with null logits); skipped_steps counts them per generation
        self.copy_cols = None
        self.copy_step = False
        self.skipped_steps = 0
        # Mirostat's state of the rows, fp32 [B] in bits, this decoder's rows (allocated once: captured graphs hold its address; None
        # until a generation asks for it); the selection kernel updates it on the columns a row draws
        self.mirostat_mu = None
        # token log-probabilities (return_logprobs=): fp32 [B, 1 + max_len], this decoder's rows; mmtg_decode_logprob writes the step's
        # column (allocated once: captured graphs hold its address)
        self.tok_lp = None
        # what _select / _logprob read: the step's own logits over every row (GuidedDecoder: the guided scores, its prompts' rows)
        self.select_rows, self.select_logits = B, None if self.children else self.logits

    def _conv1d(self, x, wkey, out, **kw):
        # bf16: Engine._fwd routes Conv1D weights through their [out,in] copies (NT layout), which is
        # what the 256x32 small-M GEMM configuration serves; the engine keeps the copies fresh.
        self.eng._fwd(x, wkey, out, self.B, "conv1d", **kw)

    # ------------------------------------------------------------------ one token
    def _step(self, with_head, parity=0):
        self.pos, self.pos_next = self.pos_pair[parity], self.pos_pair[1 - parity]
        if self.children:
            # fork: lane 0 stays on the current stream, the others run on side streams; join before the step ends
            cur = torch.cuda.current_stream()
            for st in self.side:
                st.wait_stream(cur)
            for i, ch in enumerate(self.children):
                ch.params = self.params
                if i == 0:
                    ch._step(with_head, parity)
                else:
                    with torch.cuda.stream(self.side[i - 1]):
                        ch._step(with_head, parity)
            for st in self.side:
                cur.wait_stream(st)
            return
        eng, sh, B = self.eng, self.eng.sh, self.B
        D, H, E = sh.D, sh.H, sh.E
        pre = "decoder.gpt2.transformer."
        sent = sh.msl + 2
        if self.x3:
            self._step_x3(with_head)
            self._select(with_head)
            self._logprob(with_head)
            self._end_step(with_head)
            return
        hip.decode_embed(eng.table, self.seq, self.c, self.x, self.pos, self.tpw_type, self.tpw_mask, self.types,
                         self.keep, B, sh.P, sh.S, E, sh.two_sents, eng.table.shape[0], sent,
                         sh.max_seq_length // sent + 1)
        eng._fwd(self.x, "decoder.projector_layer1.weight", self.h1, B, "linear",
                 bias=eng.P("decoder.projector_layer1.bias"), epi=hip.EPI_TANH)
        fused = self.fused
        if fused and self.embed_in_proj:
            # projector_layer2 + the GPT-2 input embedding (wpe[pos] + wte[type]) + the first LayerNorm statistics in one launch
            w2 = eng.W("decoder.projector_layer2.weight")
            hip.decode_gemm(2, self.h1, w2, self.h, B, D, H, bias=eng.P("decoder.projector_layer2.bias"), stats_out=self.st[0],
                            emb_pos=eng.W(pre + "wpe.weight"), emb_type=eng.W(pre + "wte.weight"), type_ids=self.types, pos=self.pos, ldr=D)
        else:
            eng._fwd(self.h1, "decoder.projector_layer2.weight", self.h, B, "linear", bias=eng.P("decoder.projector_layer2.bias"))
            hip.decode_embed_add(self.h, eng.W(pre + "wpe.weight"), eng.W(pre + "wte.weight"), self.types, self.pos, self.h, B, D,
                                 stats=self.st[0] if fused else None)
        hcur, hnext = self.h, self.h2
        if fused:
            self._layers_fused(hcur, hnext, with_head)
        elif self.fast:
            self._layers_split(hcur, hnext, with_head)
        else:
            self._layers_plain(hcur, hnext, with_head)
        if with_head and not fused:
            hip.gemm(self.a, eng.Wp("wte"), self.logits, B, eng.layout.Vpad, D, transB=True, ldb=D, out_f32=True)
        self._select(with_head)
        self._logprob(with_head)
        self._end_step(with_head)

    def _end_step(self, with_head):
        """What a subclass launches behind the selection and the log-probabilities of every step (GuidedDecoder: the mirror).  Here:
        nothing."""

    def _begin_lead(self, batch, length):
        """The leading positional arguments ``generate`` hands ``begin``: (batch, length) here; GuidedDecoder's begin takes the negative
        batch and the scale among them."""
        return batch, length

    def _result_rows(self):
        """How many of the decoder's rows ``generate`` returns: all of them here; GuidedDecoder's prompts, not their negatives."""
        return self.B

    def _select(self, with_head):
        """The step's last launch: logits processing + arg-max / draw + the forced cadence + the next position (generate.py:117-142),
        through the entry select_forms names: the *_fixed ones leave row b's column pos + 1 alone while pos + 1 < fixed_end[b] (the
        host wrote it), the *_ngram ones also ban every id that would complete a content n-gram the row already holds, the *_lines
        ones (n possibly 0) add the line-length bounds and line-end sets of include/mmtg_hip.h, the *_tmpl ones the line templates,
        the *_rhyme ones (templates or none) the rhyme scheme, the *_refrain ones (any of these or none) the copy lines -- also on a
        step that skipped the head because every row copies or is held (null logits: the copies and nothing else are written)."""
        sh, rules = self.eng.sh, self.rules
        temperature, rep, top_k, top_p = self.params
        form = rules.forms(with_head, self.copy_step)[0]
        B = self.select_rows
        logits, ldl, V = (self.select_logits, self.eng.layout.Vpad, min(sh.V, 13317)) if with_head else (None, 0, 0)
        if form == "_refrain":              # (the tables' shapes are held against the cut with or without logits)
            V = min(sh.V, 13317)
        # stochastic: the draw of each position reads its row of the pre-filled uniforms
        sampling = (top_k, top_p, self.uniforms) if with_head and not (top_k == 1 and top_p == 0.0) else None
        if with_head and rules.mirostat[0] > 0.0:   # Mirostat behind the four cuts (on or off): the warp entry's launch plus the rows' state
            hip.decode_sample_mirostat(logits, ldl, V, self.seq, self.pos, sh.P, sh.msl + 2, temperature, rep, top_k, top_p, rules.warp,
                                       rules.mirostat, self.mirostat_mu, self.uniforms, B, pos_next=self.pos_next,
                                       **rules.tail(self.fixed_end, "src"))
            return
        if with_head and rules.warp != WARP_OFF:    # min_p / typical_p / epsilon_cutoff / eta_cutoff: one entry over the refrain form, whatever the rules
            hip.decode_sample_warp(logits, ldl, V, self.seq, self.pos, sh.P, sh.msl + 2, temperature, rep, top_k, top_p, rules.warp,
                                   self.uniforms, B, pos_next=self.pos_next, **rules.tail(self.fixed_end, "src"))
            return
        hip._select(form, logits, ldl, V, self.seq, self.pos, sh.P, sh.msl + 2, temperature, rep, B, self.pos_next, sampling,
                    **rules.tail(self.fixed_end))

    def _logprob(self, with_head):
        """With return_logprobs, after the selection of a step that called the head: tok_lp[b, pos + 1 - P] = log_softmax of the row's
        raw logits at the id column pos + 1 now holds (include/mmtg_hip.h, mmtg_decode_logprob).  A node of its own behind the
        selection, on the same stream: it reads self.pos, which the selection leaves alone, and the selection kernels stay what they
        were.  Off, nothing is launched."""
        if self.rules.forms(with_head, self.copy_step)[2]:
            sh = self.eng.sh
            hip.decode_logprob(self.logits, self.eng.layout.Vpad, min(sh.V, 13317), self.seq, self.pos, sh.P, self.tok_lp, self.select_rows)

    def _upload_lines(self, tables):
        """The line tables into this decoder's device buffers (allocated once, so captured graphs keep their addresses; a `sets`
        buffer that has to grow drops the graphs captured on the old one).  Returns them as the *_lines entries take them, (lo, hi,
        sets or None, set_of or None) over all rows, or None without tables."""
        if tables is None:
            return None
        dev, B, sent = self.eng.dev, self.B, self.eng.sh.msl + 2
        if self._line_buf is None:
            ml = (self.max_len - 1) // sent + 1
            self._line_buf = [torch.zeros(B, ml, dtype=torch.uint8, device=dev), torch.zeros(B, ml, dtype=torch.uint8, device=dev),
                              torch.zeros(B, ml, dtype=torch.int16, device=dev), None]
        lo, hi, set_of, sets = self._line_buf
        _fill(lo, tables.lo, 0, 1)
        _fill(hi, tables.hi, sent - 2, 1)
        if tables.sets is None:
            return lo, hi, None, None
        need = tables.sets.shape[0]
        if sets is None or sets.shape[0] < need:
            cap = 16
            while cap < need:
                cap *= 2
            sets = self._line_buf[3] = torch.zeros(cap, tables.sets.shape[1], dtype=torch.int32, device=dev)
            self.graphs = {k: g for k, g in self.graphs.items()
                           if "lines" not in k and "tmpl" not in k and "rhyme" not in k and "refrain" not in k}
        _fill(sets, tables.sets.view(np.int32), 0, 0)
        _fill(set_of, tables.set_of, -1, 1)
        return lo, hi, sets, set_of

    def _upload_templates(self, tables):
        """The symbol table of a templated generation into this decoder's buffer (allocated once: captured graphs hold its address),
        lines past the generation's free (-1); None without templates."""
        if tables is None or tables.tmpl is None:
            return None
        sent = self.eng.sh.msl + 2
        if self._tmpl_buf is None:
            self._tmpl_buf = torch.zeros(self.B, (self.max_len - 1) // sent + 1, sent - 2, dtype=torch.int32, device=self.eng.dev)
        return _fill(self._tmpl_buf, tables.tmpl, -1, 1)

    def _upload_rhyme(self, tables):
        """The rhyme tables of a generation with a scheme into this decoder's buffers (allocated once: captured graphs hold their
        addresses), lines past the generation's without a leader (-1); None without a scheme.  `distinct` is a launch argument, so it
        is part of the graph key."""
        if tables is None or tables.lead is None:
            return None
        if self._rhyme_buf is None:
            sent, dev = self.eng.sh.msl + 2, self.eng.dev
            self._rhyme_buf = (torch.zeros(min(self.eng.sh.V, 13317), dtype=torch.int16, device=dev),
                               torch.zeros(self.B, (self.max_len - 1) // sent + 1, dtype=torch.int8, device=dev))
        class_of, lead = self._rhyme_buf
        _fill(class_of, tables.class_of[:class_of.shape[0]], -1, 0)
        _fill(lead, tables.lead, -1, 1)
        return class_of, lead, bool(tables.distinct)

    def _upload_refrain(self, tables):
        """The refrain table of a generation with a scheme into this decoder's buffer (allocated once: captured graphs hold its
        address), lines past the generation's no copies (-1); None without a scheme."""
        if tables is None or tables.src is None:
            return None
        if self._refrain_buf is None:
            sent = self.eng.sh.msl + 2
            self._refrain_buf = torch.zeros(self.B, (self.max_len - 1) // sent + 1, dtype=torch.int8, device=self.eng.dev)
        return _fill(self._refrain_buf, tables.src, -1, 1)

    def _copy_columns(self, tables, prefix, length, return_logprobs):
        """Which lyric columns 0 .. length skip the head under the refrain table: bool [1 + length], or None when there is nothing to
        skip.  Column j is skipped when every row is on a held prefix column or a copy column there (and one at least copies: columns
        every row holds are the prefix shortcut of ``step_at``) and no log-probabilities are asked for.  The forced cadence columns
        skip the head anyway.  MMTG_DECODE_REFRAIN_SKIP=0 keeps the head on every copy column (the ids are the same)."""
        if (tables is None or tables.src is None or return_logprobs or not self._skips_copies
                or os.environ.get("MMTG_DECODE_REFRAIN_SKIP", "1") == "0"):
            return None
        sent, src = self.eng.sh.msl + 2, tables.src
        j = np.arange(1 + length)
        line = np.minimum(j // sent, src.shape[1] - 1)
        content = (j % sent != 0) & (j % sent != sent - 1) & (j // sent < src.shape[1])
        copy = (src[:, line] >= 0) & content[None, :]                      # [B, 1 + length]
        held = np.zeros_like(copy) if prefix is None else j[None, :] < np.asarray([len(p) for p in prefix])[:, None]
        cols = (copy | held).all(0) & (copy & ~held).any(0)
        return cols if cols.any() else None

    def _step_x3(self, with_head):
        """The split-precision token step: embedding -> projector -> 12 blocks -> head, every product through mmtg_decode_gemm_x3
        on plane pairs.  Per block: c_attn (LN-fold, fp32 slabs summed by the attention kernel) -> attention over the fp32 KV cache
        (context as a plane pair) -> attn.c_proj (+ bias + fp32 residual, statistics; fp32 stream AND its plane pair) -> c_fc
        (LN-fold + GELU, plane pair) -> mlp.c_proj (as attn.c_proj); the head is an LN-fold product writing fp32 logits."""
        eng, sh, B = self.eng, self.eng.sh, self.B
        D, H, E = sh.D, sh.H, sh.E
        pre = "decoder.gpt2.transformer."
        sent = sh.msl + 2
        sq, sp, _, s2 = self.splits
        p1, p2 = self.psplits
        NP = D // 32
        hip.decode_embed_x3(eng.table, self.seq, self.c, self.xp, self.pos, self.tpw_type, self.tpw_mask, self.types,
                            self.keep, B, sh.P, sh.S, E, sh.two_sents, eng.table.shape[0], sent, sh.max_seq_length // sent + 1)
        hip.decode_gemm_x3(2, self.xp, eng.Wx("decoder.projector_layer1.weight"), B, H, E, Cp=self.h1p,
                           bias=eng.P("decoder.projector_layer1.bias"), act=hip.EPI_TANH, splits=p1, ws=self.rws, counters=self.rcnt)
        x, xo, xp, xop = self.h, self.h2, self.hp, self.h2p
        st, sto = self.st
        hip.decode_gemm_x3(2, self.h1p, eng.Wx("decoder.projector_layer2.weight"), B, D, H, C_=x, Cp=xp,
                           bias=eng.P("decoder.projector_layer2.bias"), stats_out=st, splits=p2, ws=self.rws, counters=self.rcnt,
                           emb_pos=eng.P(pre + "wpe.weight"), emb_type=eng.P(pre + "wte.weight"), type_ids=self.types, pos=self.pos, ldr=D)
        kper = -(-(-(-D // sq)) // 64) * 64
        nslab = -(-D // kper)
        for l in range(sh.L):
            p = f"{pre}h.{l}."
            wf, c, bq = self.fq[l]
            hip.decode_gemm_x3(1, xp, wf, B, 3 * D, D, C_=self.part, colsum=c, stats_in=st, np_in=NP, eps=sh.eps, splits=sq)
            hip.decode_attn_split_x3(self.part, nslab, bq, self.kc[l], self.vc[l], self.keep, self.pos, self.ctxp, B, sh.nH, 64, self.Tmax,
                                     rows=self.rows)
            hip.decode_gemm_x3(2, self.ctxp, eng.Wtx(p + "attn.c_proj.weight"), B, D, D, C_=xo, Cp=xop, bias=eng.P(p + "attn.c_proj.bias"),
                               resid=x, stats_out=sto, splits=sp, ws=self.rws, counters=self.rcnt)
            wf, c, bfc = self.ffc[l]
            hip.decode_gemm_x3(0, xop, wf, B, 4 * D, D, Cp=self.gp, bias=bfc, colsum=c, stats_in=sto, np_in=NP, eps=sh.eps, act=hip.EPI_GELU)
            hip.decode_gemm_x3(2, self.gp, eng.Wtx(p + "mlp.c_proj.weight"), B, D, 4 * D, C_=x, Cp=xp, bias=eng.P(p + "mlp.c_proj.bias"),
                               resid=xo, stats_out=st, splits=s2, ws=self.rws, counters=self.rcnt)
        if with_head:
            wf, c, bh = self.fh
            hip.decode_gemm_x3(0, xp, wf, B, eng.layout.Vpad, D, C_=self.logits, bias=bh, colsum=c, stats_in=st, np_in=NP, eps=sh.eps)

    def _layers_plain(self, hcur, hnext, with_head):
        """One GPT-2 block per layer with the training-side kernels (fp32 parity mode)."""
        eng, sh, B = self.eng, self.eng.sh, self.B
        D = sh.D
        pre = "decoder.gpt2.transformer."
        for l in range(sh.L):
            p = f"{pre}h.{l}."
            hip.layernorm_fwd(hcur, self.a, eng.P(p + "ln_1.weight"), eng.P(p + "ln_1.bias"), self.mu, self.rs, B, D, sh.eps)
            self._conv1d(self.a, p + "attn.c_attn.weight", self.qkv, bias=eng.P(p + "attn.c_attn.bias"))
            hip.decode_attn(self.qkv, self.kc[l], self.vc[l], self.keep, self.pos, self.ctx, B, sh.nH, 64, self.Tmax)
            self._conv1d(self.ctx, p + "attn.c_proj.weight", hnext, bias=eng.P(p + "attn.c_proj.bias"),
                         epi=hip.EPI_RESID, aux=hcur, ldaux=D)
            hip.layernorm_fwd(hnext, self.a, eng.P(p + "ln_2.weight"), eng.P(p + "ln_2.bias"), self.mu, self.rs, B, D, sh.eps)
            self._conv1d(self.a, p + "mlp.c_fc.weight", self.g, bias=eng.P(p + "mlp.c_fc.bias"),
                         epi=hip.EPI_GELU, aux2=self.u)
            self._conv1d(self.g, p + "mlp.c_proj.weight", hcur, bias=eng.P(p + "mlp.c_proj.bias"),
                         epi=hip.EPI_RESID, aux=hnext, ldaux=D)
        if with_head:
            hip.layernorm_fwd(hcur, self.a, eng.P(pre + "ln_f.weight"), eng.P(pre + "ln_f.bias"), self.mu, self.rs, B, D, sh.eps)

    def _split(self, x, wkey, out, splits, bias, **fin):
        """Deterministic split-K product for the batch-sized M of a decode step: `splits` K slices store
        fp32 partial products (N/32 x splits workgroups instead of N/32), splitk_finish sums them in order
        and applies bias / activation / residual (/ the next LayerNorm)."""
        self._slabs(x, wkey, splits)
        hip.splitk_finish(self.part, splits, self.B, self.eng.W(wkey).shape[1], out, bias=bias, **fin)

    def _slabs(self, x, wkey, splits):
        """`splits` fp32 partial products of x @ W into self.part (bf16: the [out,in] weight copy through the 64x64 LDS-DMA
        configuration; fp32: the Conv1D weight as stored through the fp32 kernel)."""
        if self.eng.dtype == hip.BF16:
            wt = self.eng.Wt(wkey)
            N, K = wt.shape
            hip.gemm(x, wt, self.part, self.B, N, K, transB=True, ldb=K, ldc=N, epi=hip.EPI_SPLIT, out_f32=True, splits=splits)
        else:
            w = self.eng.W(wkey)
            K, N = w.shape
            hip.gemm(x, w, self.part, self.B, N, K, ldb=N, ldc=N, epi=hip.EPI_SPLIT, out_f32=True, splits=splits)

    def _layers_split(self, hcur, hnext, with_head):
        """bf16 fast path: 4 split-K products + 4 finish kernels + attention per layer; every LayerNorm
        rides on the finish kernel of the product before it (self.a always holds the next LN output)."""
        eng, sh, B = self.eng, self.eng.sh, self.B
        D = sh.D
        pre = "decoder.gpt2.transformer."
        sq, sp, s1, s2 = self.splits
        hip.layernorm_fwd(hcur, self.a, eng.P(pre + "h.0.ln_1.weight"), eng.P(pre + "h.0.ln_1.bias"), self.mu, self.rs, B, D, sh.eps)
        for l in range(sh.L):
            p = f"{pre}h.{l}."
            if os.environ.get("MMTG_DECODE_ATTN_SPLIT", "1") == "1":
                # c_attn: the attention kernel sums the split-K slabs itself (no finish launch)
                self._slabs(self.a, p + "attn.c_attn.weight", sq)
                hip.decode_attn_split(self.part, sq, eng.P(p + "attn.c_attn.bias"), self.kc[l], self.vc[l], self.keep, self.pos,
                                      self.ctx, B, sh.nH, 64, self.Tmax, rows=self.rows)
            else:
                self._split(self.a, p + "attn.c_attn.weight", self.qkv, sq, eng.P(p + "attn.c_attn.bias"))
                hip.decode_attn(self.qkv, self.kc[l], self.vc[l], self.keep, self.pos, self.ctx, B, sh.nH, 64, self.Tmax)
            self._split(self.ctx, p + "attn.c_proj.weight", hnext, sp, eng.P(p + "attn.c_proj.bias"),
                        epi=hip.EPI_RESID, aux=hcur, ldaux=D,
                        ln_gamma=eng.P(p + "ln_2.weight"), ln_beta=eng.P(p + "ln_2.bias"), ln_out=self.a, eps=sh.eps)
            if s1 == 1:     # one K slice: bias + GELU in the product's own epilogue, no finish launch
                self._conv1d(self.a, p + "mlp.c_fc.weight", self.g, bias=eng.P(p + "mlp.c_fc.bias"), epi=hip.EPI_GELU, aux2=self.u)
            else:
                self._split(self.a, p + "mlp.c_fc.weight", self.g, s1, eng.P(p + "mlp.c_fc.bias"), epi=hip.EPI_GELU)
            if l + 1 < sh.L:
                nxt = f"{pre}h.{l + 1}.ln_1."
            else:
                nxt = pre + "ln_f." if with_head else None
            ln = {} if nxt is None else dict(ln_gamma=eng.P(nxt + "weight"), ln_beta=eng.P(nxt + "bias"), ln_out=self.a, eps=sh.eps)
            self._split(self.g, p + "mlp.c_proj.weight", hcur, s2, eng.P(p + "mlp.c_proj.bias"),
                        epi=hip.EPI_RESID, aux=hnext, ldaux=D, **ln)

    def _refresh_folds(self):
        """gamma-folded weight copies, their column sums and folded biases for the LN-fold products (once per generation: the
        weights may have been stepped)."""
        eng, sh = self.eng, self.eng.sh
        D = sh.D
        pre = "decoder.gpt2.transformer."
        if self.x3:
            for l in range(sh.L):
                p = f"{pre}h.{l}."
                wf, c, b = self.fq[l]
                hip.ln_fold_weights_x3(eng.Wtx(p + "attn.c_attn.weight"), eng.P(p + "ln_1.weight"), eng.P(p + "ln_1.bias"),
                                       eng.P(p + "attn.c_attn.bias"), wf, c, b, 3 * D, D)
                wf, c, b = self.ffc[l]
                hip.ln_fold_weights_x3(eng.Wtx(p + "mlp.c_fc.weight"), eng.P(p + "ln_2.weight"), eng.P(p + "ln_2.bias"),
                                       eng.P(p + "mlp.c_fc.bias"), wf, c, b, 4 * D, D)
            wf, c, b = self.fh
            hip.ln_fold_weights_x3(eng.Wpx("wte", eng.layout.Vpad, D), eng.P(pre + "ln_f.weight"), eng.P(pre + "ln_f.bias"), None, wf, c, b,
                                   eng.layout.Vpad, D)
            return
        for l in range(sh.L):
            p = f"{pre}h.{l}."
            wf, c, b = self.fq[l]
            hip.ln_fold_weights(eng.Wt(p + "attn.c_attn.weight"), eng.P(p + "ln_1.weight"), eng.P(p + "ln_1.bias"),
                                eng.P(p + "attn.c_attn.bias"), wf, c, b, 3 * D, D)
            wf, c, b = self.ffc[l]
            hip.ln_fold_weights(eng.Wt(p + "mlp.c_fc.weight"), eng.P(p + "ln_2.weight"), eng.P(p + "ln_2.bias"),
                                eng.P(p + "mlp.c_fc.bias"), wf, c, b, 4 * D, D)
        wf, c, b = self.fh
        hip.ln_fold_weights(eng.Wp("wte"), eng.P(pre + "ln_f.weight"), eng.P(pre + "ln_f.bias"), None, wf, c, b, eng.layout.Vpad, D)

    def _layers_fused(self, hcur, hnext, with_head):
        """bf16 fused path: per block c_attn (LN-fold, split-K slabs summed by the attention kernel) -> attention -> attn c_proj
        (split-K reduced in the kernel + bias + residual + statistics) -> c_fc (LN-fold + GELU) -> mlp c_proj (as c_proj); the
        head is an LN-fold product writing fp32 logits.  The residual stream alternates between two buffers and so do its
        LayerNorm statistics.  (Round 4's persistent one-launch step and chained launches -- bit-equal, measured slower -- are kept as
        tools/experiments/decode_persistent_and_chained.patch.)"""
        eng, sh, B = self.eng, self.eng.sh, self.B
        D = sh.D
        pre = "decoder.gpt2.transformer."
        sq, sp, _, s2 = self.splits
        NP = D // 32
        kper = -(-(-(-D // sq)) // 64) * 64          # K slices are whole 64-deep tiles: the product writes ceil(D / kper) slabs
        nslab = -(-D // kper)
        x, xo = hcur, hnext
        st, sto = self.st
        mlp = self.mlp
        npx = NP            # statistics partials of the block's input rows (the projector's / a mode-2 product's: one per 32 columns)
        for l in range(sh.L):
            p = f"{pre}h.{l}."
            wf, c, bq = self.fq[l]
            hip.decode_gemm(1, x, wf, self.part, B, 3 * D, D, colsum=c, stats_in=st, np_in=npx, eps=sh.eps, out_f32=True, splits=sq)
            hip.decode_attn_split(self.part, nslab, bq, self.kc[l], self.vc[l], self.keep, self.pos,
                                  self.ctx, B, sh.nH, 64, self.Tmax, rows=self.rows)
            hip.decode_gemm(2, self.ctx, eng.Wt(p + "attn.c_proj.weight"), xo, B, D, D, bias=eng.P(p + "attn.c_proj.bias"), resid=x,
                            stats_out=sto, splits=sp, ws=self.rws, counters=self.rcnt)
            wf, c, bfc = self.ffc[l]
            if mlp:
                # c_fc (LN-fold + GELU) -> mlp.c_proj (+ bias + residual + statistics, 16 partials of 48 columns) in one launch
                hip.decode_mlp(xo, sto, NP, sh.eps, wf, c, bfc, eng.Wt(p + "mlp.c_proj.weight"), eng.P(p + "mlp.c_proj.bias"), self.g, x, st,
                               self.mlp_ws, self.mlp_sync, B, D, plain=self.mlp_plain, trace=self.mlp_trace)
                npx = 16
                continue
            hip.decode_gemm(0, xo, wf, self.g, B, 4 * D, D, bias=bfc, colsum=c, stats_in=sto, np_in=NP, eps=sh.eps, act=hip.EPI_GELU)
            hip.decode_gemm(2, self.g, eng.Wt(p + "mlp.c_proj.weight"), x, B, D, 4 * D, bias=eng.P(p + "mlp.c_proj.bias"), resid=xo,
                            stats_out=st, splits=s2, ws=self.rws, counters=self.rcnt)
        if with_head:
            wf, c, bh = self.fh
            hip.decode_gemm(0, x, wf, self.logits, B, eng.layout.Vpad, D, bias=bh, colsum=c, stats_in=st, np_in=npx, eps=sh.eps,
                            out_f32=True)

    def _run_step(self, with_head, parity):
        if not self.use_graph:
            self._step(with_head, parity)
            return
        key = self._graph_key(with_head, parity)
        g = self.graphs.get(key)
        if g is None:
            # warm-up outside capture (lazy LDS-attribute / module loading), then rewind the position
            state = self._step_state()
            saved = [t.clone() for t in state]
            self._step(with_head, parity)
            torch.cuda.synchronize()
            for t, v in zip(state, saved):
                t.copy_(v)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step(with_head, parity)
            self.graphs[key] = g
            for t, v in zip(state, saved):
                t.copy_(v)
        g.replay()

    def _graph_key(self, with_head, parity):
        """What the step's launches depend on: the settings, and the rules as far as they reach this step (StepRules.key)."""
        return (with_head, parity, self.params) + self.rules.key(with_head, self.copy_step)

    def _step_state(self):
        """What a token step changes besides the caches' slot `pos` (rewound around the warm-up step of a graph capture).  With
        Mirostat that includes the rows' mu: without it the first step of every new graph key would update mu twice."""
        return [self.pos_all, self.seq, self.keep] + ([self.mirostat_mu] if self.rules.mirostat[0] > 0.0 else [])

    # ------------------------------------------------------------------ public
    def describe(self):
        how = "one hipGraph replay per token step" if self.use_graph else "eager launches per token step"
        return how + (", %d row blocks of %d side by side" % (self.lanes, self.B // self.lanes) if self.lanes > 1 else "")

    def kernel_name(self):
        if self.x3:
            return ("decode token step (bf16x3): decode_gemm_x3_kernel<64x64> weight streaming over (hi | lo) plane pairs, three bf16 matrix-core "
                    "passes per product (split-K reduced in the kernel, LayerNorm applied algebraically, fp32 residual stream) + decode_attn "
                    "streaming an fp32 KV cache, 5 graph nodes per block")
        if self.fused and self.mlp:
            return ("decode token step: decode_gemm_kernel<64x64> weight streaming (c_attn LN-fold slabs, attn.c_proj split-K reduced in the "
                    "kernel) + decode_attn KV-cache streaming + decode_mlp_kernel (c_fc -> GELU -> mlp.c_proj in one launch, hidden dimension "
                    "split over the XCDs, %s hand-off), 4 graph nodes per block" % ("L2" if self.mlp_plain else "write-through"))
        if self.fused:
            return ("decode token step: decode_gemm_kernel<64x64> weight streaming (split-K reduced in the kernel, LayerNorm applied "
                    "algebraically) + decode_attn KV-cache streaming, 5 graph nodes per block")
        return ("decode token step: split-K gemm_dma_kernel<64x64> weight streaming + decode_attn KV-cache streaming + finish kernels"
                if self.fast else "decode token step: training-side kernels per layer")

    @torch.no_grad()
    def begin(self, batch, length, temperature=1.0, repitition_penalty=1.0, top_k=1, top_p=0.0, generator=None, prefix=None,
              no_repeat_ngram_size=0, line_lengths=None, line_end_ids=None, templates=None, rhyme_scheme=None, rhyme_classes=None,
              rhyme_distinct=False, return_logprobs=False, keywords=None, refrain_scheme=None, min_p=0.0, typical_p=1.0,
              epsilon_cutoff=0.0, eta_cutoff=0.0, mirostat_tau=0.0, mirostat_eta=0.1, _search=None):
        """Everything of a generation that happens once: the settings, the uniforms of a stochastic run, fresh weight copies /
        LayerNorm folds, the experience encoder, the prompt (prefilled in one batched pass: ``first_pos`` = P afterwards) and the
        reset position.  Returns the end position n; ``step_at(pos)`` for pos = first_pos .. n - 1 then runs the token steps (``generate`` does both; tools/decode_lanes_threads.py drives
        several decoders' steps from their own threads and streams).

        prefix (optional; check_prefix states the rules): row b's first L_b lyric ids, written into seq[b, P:P + L_b] with
        fixed_end[b] = P + L_b -- the steps leave those columns alone.  The prefill then covers [prompt, p[:, :Lmin]] (Lmin = min_b
        L_b, first_pos = P + Lmin - 1); longer prefixes go through token steps held by fixed_end.  prefix=None runs exactly the
        launches and graphs of an unprefixed generation.

        no_repeat_ngram_size (check_ngram): n > 0 makes every step that calls the head end in the *_ngram selection entries, so no
        row writes a content n-gram it already holds (prefix columns count as history).  0 runs exactly the launches and graphs of a
        generation without the argument.

        line_lengths / line_end_ids (check_lines states the forms and the rule's home is include/mmtg_hip.h): per-row, per-line
        bounds on the number of content tokens and sets the last content token of a line comes from.  With either given, every
        step that calls the head ends in the *_lines selection entries; the tables are uploaded here, once.  None for both runs
        exactly the launches and graphs of a generation without them.  (line_lengths may also be a LineTables, taken as checked.)

        templates (check_lines states the forms, include/mmtg_hip.h the rule): given ids, free columns and id classes for the opening
        columns of a line.  With templates every step that calls the head ends in the *_tmpl selection entries; the symbol table is
        uploaded here, once, beside the line tables.  None runs exactly the launches and graphs of a generation without them.

        rhyme_scheme / rhyme_classes / rhyme_distinct (check_lines states the forms, include/mmtg_hip.h the rule): which lines end on
        one rhyme, e.g. "AABB", over the caller's partition of the ids that have a rhyme; which rhyme is each row's own choice,
        made when it ends the group's first line.  With a scheme every step that calls the head ends in the *_rhyme selection
        entries; the tables are uploaded here, once.  None runs exactly the launches and graphs of a generation without it.

        return_logprobs: keep ``tok_lp`` fp32 [B, 1 + max_len], zeroed here: every step that calls the head then ends in one more
        launch, mmtg_decode_logprob, which writes column j of the step -- the log-probability the model's raw logits (no penalty, no
        temperature, no bans; cut at 13317) give the id the column holds after the selection, whoever decided it: the model's pick, a
        draw, a template's given id, a full line's PAD, a sticky PAD or a held prefix id.  Column 0, the forced [#START#] / [#EOS#]
        columns and every step that skips the head stay 0.  No step skips the head because every row is held by its prefix (the
        shortcut of ``step_at``), so held columns carry the given id's log-probability.  Scoring mode: when every row's prefix is
        the whole row (1 + length ids), the prefill covers the prompt only and every content column goes through a token step --
        teacher forcing through the kernels that generate.  A shorter prefix keeps the prefill of the generation without the
        argument (its ids are bit-equal to that generation's), and the columns the prefill covers stay 0.  False runs exactly the
        launches, graphs and graph keys of a generation without the argument.

        refrain_scheme (check_refrain states the forms, include/mmtg_hip.h the rule): which lines repeat an earlier line of the row,
        e.g. "AB.A" (line 3 is line 0 again, whatever the model wrote there).  With a scheme every step that calls the head ends in
        the *_refrain selection entries (the rhyme form plus the copy, with whatever other rules there are or none); src is uploaded
        here, once.  A step at which every row sits on a held prefix column or a copy column calls no head at all (``step_at``; not
        with return_logprobs, which wants the head's word on every column): it ends in mmtg_decode_select_refrain with null logits.
        The uniforms of a sampled generation are indexed by position, so a skipped draw consumes nothing.  ``skipped_steps`` counts
        those steps; MMTG_DECODE_REFRAIN_SKIP=0 (read here) keeps the head on them, with the same ids.  None runs exactly the
        launches, graphs and graph keys of a generation without the argument.

        min_p / typical_p / epsilon_cutoff / eta_cutoff (check_warp states the ranges, include/mmtg_hip.h the rule,
        constraints.warp_filter restates it): four more truncation stages of the draw, behind top_k / top_p, with the names and defaults
        of transformers' generate.  With any of them on, the generation samples (uniforms are drawn, also at top_k=1, top_p=0, where the
        top-1 filter leaves the stages nothing to do) and every step that calls the head ends in mmtg_decode_sample_warp, whatever
        constraints there are; the values join the graph key.  A step without the head runs what it always ran.  All four at their
        defaults run exactly the launches, graphs and graph keys of a generation without the arguments.

        mirostat_tau / mirostat_eta (check_mirostat states the ranges, include/mmtg_hip.h the rule, constraints.mirostat_filter and
        mirostat_update restate it): Mirostat v2 as the last stage of the draw, behind top_k / top_p and the four above, with llama.cpp's
        names.  mirostat_tau > 0 turns it on: the generation samples (uniforms are drawn, also at top_k=1, top_p=0), every step that
        calls the head ends in mmtg_decode_sample_mirostat, whatever the other values and constraints, and ("mirostat", tau, eta) joins
        the graph key.  The rows' state ``mirostat_mu`` (fp32 [B], bits) is filled with 2 * tau here and readable after the generation;
        only a column that a row draws changes its entry.  mirostat_tau=0 runs exactly the launches, graphs and graph keys of a
        generation without the arguments, and allocates nothing.

        keywords: refused here (ValueError).  A lyric that contains given words needs a search, and greedy decoding and sampling
        follow one path: BeamDecoder takes keywords=.

        _search: the StepRules fields a search decoder decides (BeamDecoder.begin: groups, diversity_penalty, kw), for the one
        record built here."""
        _keywords_need_beams(keywords)
        warp = check_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)
        mirostat = check_mirostat(mirostat_tau, mirostat_eta)
        miro_on = mirostat[0] > 0.0
        eng, sh = self.eng, self.eng.sh
        B = batch["img_embs"].shape[0]
        if B != self.B:
            raise ValueError("decoder was built for batch %d, got %d" % (self.B, B))
        if length > self.max_len:
            raise ValueError("length %d exceeds max_len %d" % (length, self.max_len))
        cons = _check_constraints(prefix, no_repeat_ngram_size, line_lengths, line_end_ids, B, length, sh, "a batch of %d" % B,
                                  templates, rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme)
        pre = cons.prefix
        self.params = (float(temperature), float(repitition_penalty), int(top_k), float(top_p))
        if not (int(top_k) == 1 and float(top_p) == 0.0) or warp != WARP_OFF or miro_on:
            if self.uniforms is None:
                self.uniforms = torch.empty(sh.P + self.max_len + 1, self.B, device=eng.dev, dtype=torch.float32)
            self.uniforms.uniform_(0.0, 1.0, generator=generator)
            self.uniforms.clamp_(max=1.0 - 2.0 ** -24)
            for i, ch in enumerate(self.children):      # a lane reads its own [position, row] block of the same draws
                blk = self.uniforms[:, i * ch.B:(i + 1) * ch.B]
                if ch.uniforms is None:
                    ch.uniforms = torch.empty_like(blk, memory_format=torch.contiguous_format)
                ch.uniforms.copy_(blk)
        if self.mlp:
            self.mlp_sync.zero_()           # counters armed, error report cleared (check_mlp_error reads it after the generation)
        eng.invalidate_copies()
        self.eng.refresh_copies()
        for d in ([self] + self.children):          # (a lane has its own folded copies: they are part of its scratch)
            if d.fused or d.x3:
                d._refresh_folds()
        self.seq.zero_()
        self.seq[:, :sh.P] = batch["topic_ids"].to(eng.dev).long()
        self.seq[:, sh.P] = 1                                   # [#START#]
        lmin = 1
        if return_logprobs:
            if self.tok_lp is None:
                self.tok_lp = torch.zeros(B, 1 + self.max_len, dtype=torch.float32, device=eng.dev)
            self.tok_lp.zero_()
        self.copy_cols = self._copy_columns(cons.lines, pre, length, return_logprobs)
        if miro_on:
            if self.mirostat_mu is None:
                self.mirostat_mu = torch.empty(B, dtype=torch.float32, device=eng.dev)
            self.mirostat_mu.fill_(2.0 * mirostat[0])
        if (warp != WARP_OFF or miro_on) and self._warp_buf is None:         # the "no copy line" src of a generation without a refrain scheme
            self._warp_buf = torch.full((B, (self.max_len - 1) // (sh.msl + 2) + 1), -1, dtype=torch.int8, device=eng.dev)
        self.skipped_steps = 0
        # the generation's rules, on the decoder and its lanes: a lane's _select reads the record of its own rows (the sets are shared),
        # its slice of fixed_end (a view since construction) and its rows of the state
        bare = cons.lines is not None and cons.lines.bare       # (tables made for a refrain alone: no line rule to upload)
        self.rules = StepRules(prefix=pre is not None, ngram=cons.ngram, lines=self._upload_lines(None if bare else cons.lines),
                               tmpl=self._upload_templates(cons.lines), rhyme=self._upload_rhyme(cons.lines),
                               refrain=self._upload_refrain(cons.lines), warp=warp, warp_src=self._warp_buf,
                               mirostat=mirostat if miro_on else MIROSTAT_OFF, return_logprobs=bool(return_logprobs), **(_search or {}))
        self.copy_step = False
        for i, ch in enumerate(self.children):
            a, z = i * ch.B, (i + 1) * ch.B
            ch.rules, ch.copy_step = self.rules.rows(a, z), False
            if miro_on:
                ch.mirostat_mu = self.mirostat_mu[a:z]
            if return_logprobs:
                ch.tok_lp = self.tok_lp[a:z]
        self.min_fixed = 0
        if pre is not None:
            lens = [len(p) for p in pre]
            # (scoring mode, and a decoder that wants every lyric column from a token step: the prompt only)
            lmin = 1 if (return_logprobs and min(lens) == length + 1) or self._prefill_prompt_only else min(lens)
            host = torch.zeros(B, max(lens), dtype=torch.long)
            for b, p in enumerate(pre):
                host[b, :len(p)] = torch.tensor(p, dtype=torch.long)
            self.seq[:, sh.P:sh.P + host.shape[1]] = host.to(eng.dev)
            self.fixed_end.copy_(torch.tensor(lens, dtype=torch.int32) + sh.P)
            self.min_fixed = sh.P + lmin
        self.tpw_type.copy_(batch["tpw_type_ids"].to(eng.dev).long())
        self.tpw_mask.copy_(batch["tpw_attention_mask"].to(eng.dev).long())
        self.keep.zero_()
        self.pos_all.zero_()
        self.first_pos = 0
        if self.prefill and sh.P > 0:
            self._prefill(batch, lmin)
        else:
            a = eng.forward(batch, train_flag=False, training=False, encode_only=True)
            self.c.copy_(a["c"])
        return sh.P + length                                    # positions first_pos .. P+length-1 are consumed by token steps

    def _prefill(self, batch, lmin=1):
        """The P prompt positions in ONE batched pass instead of P token steps (a token step costs the same whatever it appends; the
        reference has no such distinction -- its every call re-runs the whole prefix, generate.py:124).  The engine's inference-branch
        forward (model.py:290-326) over [prompt, [#START#]] computes every block's K / V rows for all prompt positions at once
        (B x (P + 1) rows through the training-side kernels of the compute mode, nothing of the last block beyond its c_attn; causal,
        so the rows of the P prompt positions do not depend on the extra one -- the conditioning kernel wants at least one lyric
        position); they go into the caches, the key mask of the prompt is the prompt's attention mask, and the token
        steps start at position P.
        With a prefix the pass runs over [prompt, p[:, :lmin]] (the prefix every row has): the caches take the first P + lmin - 1
        positions, a lyric position's key mask is tok != 0 (the inference-branch rule of decode_embed) and the steps start at
        P + lmin - 1."""
        eng, sh = self.eng, self.eng.sh
        P = sh.P
        n = P + lmin - 1                                        # positions whose K / V the pass provides
        pb = dict(batch)
        pb["targets"] = self.seq[:, P:P + lmin]
        a = eng.forward(pb, train_flag=False, training=False, per_row_infer=True, need_logits=False)
        self.c.copy_(a["c"])
        B, T, nH = a["B"], a["T"], sh.nH
        for l, rec in enumerate(a["layers"]):
            qkv = rec[4]
            if isinstance(qkv, hip.Planes):        # bf16x3: c_attn writes a (hi | lo) plane pair [2, M, 3D]; the cache holds fp32 rows
                hi, lo = qkv.t[0].view(B, T, 3, nH, 64), qkv.t[1].view(B, T, 3, nH, 64)
                kv = hi[:, :n, 1:3].float() + lo[:, :n, 1:3].float()           # [B, n, 2, nH, 64]: only what the cache takes
                k, v = kv[:, :, 0], kv[:, :, 1]
            else:
                qkv = qkv.view(B, T, 3, nH, 64)
                k, v = qkv[:, :n, 1], qkv[:, :n, 2]
            self.kc[l][:, :, :n].copy_(k.permute(0, 2, 1, 3))
            self.vc[l][:, :, :n].copy_(v.permute(0, 2, 1, 3))
        self.keep[:, :P] = (self.tpw_mask != 0).to(torch.int32)
        if n > P:
            self.keep[:, P:n] = (self.seq[:, P:n] != 0).to(torch.int32)
        self.pos_all.fill_(n)
        self.first_pos = n

    def step_at(self, pos):
        """Token step `pos` of the generation ``begin`` prepared; returns whether the step called the model's head."""
        sh = self.eng.sh
        j = pos + 1 - sh.P                                      # lyric index appended after this step
        forced = j < 1 or (j > 1 and (j + 1) % (sh.msl + 2) in (0, 1))
        if self.rules.prefix and pos + 1 < self.min_fixed and not self.rules.return_logprobs:
            forced = True                                       # every row's column pos + 1 is a prefix id: no model call
        copies = bool(not forced and self.copy_cols is not None and 0 <= j < len(self.copy_cols) and self.copy_cols[j])
        if copies:                                              # every row copies or is held: no model call, the selection copies
            forced = True
            self.skipped_steps += 1
        for d in [self] + self.children:
            d.copy_step = copies
        self._run_step(with_head=not forced, parity=pos & 1)
        return not forced

    @torch.no_grad()
    def generate(self, batch, length, temperature=1.0, repitition_penalty=1.0, top_k=1, top_p=0.0, generator=None,
                 use_graph=None, teacher=None, tap=None, prefix=None, no_repeat_ngram_size=0, line_lengths=None, line_end_ids=None,
                 templates=None, rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, return_logprobs=False,
                 refrain_scheme=None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, mirostat_tau=0.0, mirostat_eta=0.1,
                 **begin_kw):
        """batch: dict with topic_ids/tpw_* [B,P], topic_emb, img_embs, r_embs (no targets needed).
        Runs `length` iterations of the reference loop and returns the lyric ids
        [B, 1 + length] (column 0 is the initial [#START#]).  top_k = 1, top_p = 0 is the greedy setting;
        anything else samples on the device (generate.py:137-141): one uniform per row and position is drawn
        from `generator` (a CUDA torch.Generator; default: the global one) before the steps are replayed.
        Parity hooks (tests/test_decode_gpu.py): `teacher` [B, 1 + length] long -- after every step the token the step
        appended is replaced by teacher[:, j] wherever that is >= 0 (teacher forcing on a reference id list; the step's own
        pick is handed to `tap` first); `tap(j, with_head, picked [B], logits [B, Vpad] or None)` is called after every step.
        prefix: the opening lyric ids of every row (``begin``, ``check_prefix``); columns 0 .. L_b - 1 of row b's result are its
        prefix, the rest follows the rules above (the penalty counts the prefix).
        no_repeat_ngram_size: n > 0 bans, at every model-chosen column, each id that would repeat a content n-gram of the row
        (``begin``, include/mmtg_hip.h); 0 (the default) is off.
        line_lengths / line_end_ids: the form of the lyric (``check_lines``): line_lengths=7 makes every line seven content
        tokens long, line_lengths=(1, 20) forbids empty lines, line_end_ids=[None, ids, None, ids] ends lines 1 and 3 on one of
        ids.  A line is full at its hi (the row pads from there), cannot end below its lo, and with an end set ends on a member.
        templates: what the opening columns of a line hold (``check_lines``): templates=[(a, ...), (b, ...)] opens line 0 with id
        a and line 1 with id b (an acrostic), (a, None, None, b) is a four-token line a ? ? b, a set in place of an id confines
        the column to its members.
        rhyme_scheme / rhyme_classes / rhyme_distinct: lines that end on one rhyme (``check_lines``): rhyme_scheme="AABB" with
        rhyme_classes=[ids that rhyme, ...] makes lines 0 / 1 and 2 / 3 end in one class each, the class being what the row ended
        the first line of the pair on; rhyme_distinct=True keeps a line from ending on the id an earlier line of its group ended on.
        refrain_scheme: lines that repeat a line (``check_refrain``): refrain_scheme="AB.A" makes line 3 the text of line 0 again,
        copied column by column from the row's own history -- also under no_repeat_ngram_size, which otherwise forbids a chorus.
        return_logprobs: return (ids, tok_lp [B, 1 + length] fp32) -- per column the log-probability the model's raw logits give the
        id the column holds, 0 where no step called the head (``begin``; ``chosen_mask`` / ``sequence_scores`` turn them into a
        score per row).  With a prefix that covers every row whole it scores given text (generate.score_sequences).
        min_p / typical_p / epsilon_cutoff / eta_cutoff: min-p, locally typical, epsilon and eta sampling (``begin``), transformers'
        arguments of those names: typical_p=0.9 keeps the ids whose surprise is nearest the entropy, min_p=0.05 drops what is under
        a twentieth of the best id's probability.  They act behind top_k / top_p, so top_k=0, top_p=0 leaves the choice to them.
        mirostat_tau / mirostat_eta: Mirostat v2 (``begin``), llama.cpp's arguments of those names: mirostat_tau=2.0 holds the observed
        surprise of the text near 2 bits per drawn token by adapting the cut after every draw, at learning rate mirostat_eta.  It acts
        last, so top_k=0, top_p=0 leaves the choice to it.  Afterwards ``mirostat_mu`` holds every row's state.
        begin_kw: what a subclass's ``begin`` takes beyond these (BeamDecoder: the beam groups); ``begin`` here takes none.  Every
        argument above goes to ``begin`` by name, at its default too: a search decoder's ``begin`` runs them through its refusals."""
        n_steps = self.begin(*self._begin_lead(batch, length), temperature=temperature, repitition_penalty=repitition_penalty, top_k=top_k,
                             top_p=top_p, generator=generator, prefix=prefix, no_repeat_ngram_size=no_repeat_ngram_size,
                             line_lengths=line_lengths, line_end_ids=line_end_ids, templates=templates, rhyme_scheme=rhyme_scheme,
                             rhyme_classes=rhyme_classes, rhyme_distinct=rhyme_distinct, return_logprobs=return_logprobs,
                             refrain_scheme=refrain_scheme, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff,
                             eta_cutoff=eta_cutoff, mirostat_tau=mirostat_tau, mirostat_eta=mirostat_eta, **begin_kw)
        eng, sh = self.eng, self.eng.sh
        saved_mode = self.use_graph
        if use_graph is not None:
            self.use_graph = use_graph
        try:
            if teacher is not None and self.first_pos > 0:          # (the prompt steps a prefill skipped would have placed column 0)
                col = teacher[:, 0].to(eng.dev)
                self.seq[:, sh.P] = torch.where(col >= 0, col, self.seq[:, sh.P])
            for pos in range(self.first_pos, n_steps):
                with_head = self.step_at(pos)
                j = pos + 1 - sh.P                                  # lyric index appended by this step
                if tap is not None:
                    tap(j, with_head, self.seq[:, pos + 1].clone(), self.logits if with_head and not self.children else None)
                if teacher is not None and 0 <= j <= length:
                    col = teacher[:, j].to(eng.dev)
                    self.seq[:, pos + 1] = torch.where(col >= 0, col, self.seq[:, pos + 1])
        finally:
            self.use_graph = saved_mode
        self.check_mlp_error()
        n = self._result_rows()
        ids = self.seq[:n, sh.P:sh.P + 1 + length].clone()
        return (ids, self.tok_lp[:n, :1 + length].clone()) if return_logprobs else ids

    def check_mlp_error(self):
        """Raise if a mmtg_decode_mlp launch of this generation reported a bounded wait that ran out or a hand-off group split over
        two XCDs (include/mmtg_hip.h): its results are undefined then.  One device read (the ids are read right after anyway)."""
        if self.mlp:
            code = int(self.mlp_sync[65].item())
            if code:
                raise RuntimeError("mmtg_decode_mlp reported error %d (2: a wait ran into its 4 ms bound -- the 256 workgroups were not "
                                   "co-resident; 4: a hand-off group sat on two XCDs in the plain mode); set MMTG_DECODE_MLP=0" % code)

    @staticmethod
    def reference_return(ids_row, length, sent=22):
        """What the reference's sample_sequence returns for one row: the sequence as it stood
        before the append of the last iteration that called the model (generate.py:126,144)."""
        last_call = max(i for i in range(length) if not (i > 0 and (i + 2) % sent in (0, 1)))
        return list(ids_row[:1 + last_call])


# ---------------------------------------------------------------------- what a search refuses
# The search decoders' begin / generate name what they add or use and take the rest as **settings.  What a search cannot honour is
# refused by a table, (names, whether their values are all "off", the reason) per row, before any device work and before anything of
# `self` is read; the rest is forwarded towards GreedyDecoder's explicit signatures, which document the arguments.
_SETTINGS = frozenset(inspect.signature(GreedyDecoder.generate).parameters) - {"self", "batch", "length", "teacher", "tap", "begin_kw"}
_WARP_NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
_MIROSTAT_NAMES = ("mirostat_tau", "mirostat_eta")
_DRAW_NAMES = ("top_k", "top_p", "generator")


def _no_draw(top_k=1, top_p=0.0, generator=None):
    return int(top_k) == 1 and float(top_p) == 0.0 and generator is None


def _no_warp(**cuts):
    return check_warp(**cuts) == WARP_OFF


def _no_mirostat(**tau_eta):
    return check_mirostat(**tau_eta)[0] == 0.0        # (eta alone turns nothing on)


def _run_refusals(table, settings):
    """`settings` through a search decoder's refusal table: TypeError for a name that neither a row of the table nor
    GreedyDecoder.generate knows (as Python's own check of an explicit signature), ValueError with the row's reason for a value that
    is not "off" (an out-of-range value is said first, by check_warp / check_mirostat).  Returns the settings without the table's
    names -- they are at their defaults -- for the caller to forward."""
    named = {k for names, _, _ in table for k in names}
    for k in settings:
        if k not in named and k not in _SETTINGS:
            raise TypeError("got an unexpected keyword argument %r" % k)
    for names, off, reason in table:
        given = {k: settings[k] for k in names if k in settings}
        if given and not off(**given):
            raise ValueError(reason)
    return {k: v for k, v in settings.items() if k not in named}


class BeamDecoder(GreedyDecoder):
    """Beam search on the KV-cached, graph-replayed token step: `num_beams` rows per prompt advance in lock step, and the step's
    last two launches (mmtg_decode_beam_candidates, mmtg_decode_beam_merge) replace decode_select.

    Per model call, candidate (beam, v) scores cum[beam] + log_softmax(x)[v] in fp32, x the beam's processed logits exactly as the
    greedy step computes them (per-occurrence repetition penalty, temperature, bans; cut at 13317); each prompt keeps its best
    `num_beams` by (score descending, parent beam ascending, rank inside the parent: x descending, id ascending), so one beam
    picks what greedy picks.  Forced [#EOS#] / [#START#] positions and sticky PAD keep the score; a PAD-terminated beam keeps its
    frozen score (no length penalty, no early stop: every beam has the same length).  Beam scores start at [0, -inf, ...], so the
    replicated beams of a prompt never yield duplicate hypotheses.  With `num_beam_groups` > 1 (``begin``) the beams are groups
    that search on their own, each started at [0, -inf, ...], a later group steered away from the ids earlier groups take at the
    same step by `diversity_penalty`; the scores stay the unpenalised sums described here.

    The KV cache is never copied: a row writes its new K / V into its own slot `pos`, and the ancestry table `rows` [B, Tmax]
    (rows[b, j] = the cache row holding position j of beam b's history) is reordered with seq / keep by the merge; the attention
    reads the prefix through it (mmtg_decode_attn_split_rows / mmtg_decode_attn_split_x3_rows)."""

    _skips_copies = False           # the merge knows nothing of copies: the candidates offer them, on a step with the head

    def __init__(self, model, max_prompts, num_beams, max_len=None, use_graph=True, lanes=1):
        nb = int(num_beams)
        if not 1 <= nb <= 16:
            raise ValueError("num_beams %d outside 1..16" % nb)
        if lanes != 1:
            raise ValueError("beam search runs on one lane (got lanes=%r)" % (lanes,))
        super().__init__(model, int(max_prompts) * nb, max_len=max_len, use_graph=use_graph, lanes=1)
        if not self.fast:
            raise ValueError("beam search needs the split decode step (MMTG_DECODE_PLAIN has no table-aware attention)")
        if not (self.x3 or self.fused) and os.environ.get("MMTG_DECODE_ATTN_SPLIT", "1") != "1":
            raise ValueError("beam search needs the split attention (MMTG_DECODE_ATTN_SPLIT=0 has no table-aware attention)")
        dev = self.eng.dev
        self.nb, self.n_prompts = nb, int(max_prompts)
        self.rows = torch.zeros(self.B, self.Tmax, dtype=torch.int32, device=dev)
        self.scores = torch.zeros(self.B, dtype=torch.float32, device=dev)
        self.cand_val = torch.zeros(self.B, nb, dtype=torch.float32, device=dev)
        self.cand_id = torch.zeros(self.B, nb, dtype=torch.int32, device=dev)
        # keywords=: the two tables of StepRules.kw, the wide candidate storage and the rhyme form's empty tables: allocated once
        self._kw_buf = None
        self._kw_cand = None        # (cand_val, cand_id, cand_bank) [B, nb + K]: views of that storage

    def _select(self, with_head):
        """The step's last two launches, through the entries select_forms names: the bans (and a full line's PAD, offered as sticky
        PAD is) act in the candidates; the merge is the prefix-aware one or the plain one -- with beam groups, on a step with the
        head, the grouped one of either (the candidates do not know of groups)."""
        sh, rules = self.eng.sh, self.rules
        temperature, rep, _, _ = self.params
        cand, merge, _ = rules.forms(with_head)
        fe = self.fixed_end if rules.prefix else None
        if cand == "_kw":
            # the rhyme form serves every rule or none; line tables without a scheme get a lead table that names no leader
            cv, ci, cb = self._kw_cand
            hip.decode_beam_candidates_kw(self.logits, self.eng.layout.Vpad, min(sh.V, 13317), self.seq, self.pos, sh.P, sh.msl + 2,
                                          temperature, rep, self.nb, cv, ci, cb, self.B, rules.kw, **rules.tail(self.fixed_end, "kw", self._kw_buf[3]))
            hip.decode_beam_merge_kw(cv, ci, cb, self.scores, self.seq, self.keep, self.rows, self.pos, sh.P, sh.msl + 2, self.nb,
                                     self.n_prompts, rules.kw[2], fixed_end=fe, pos_next=self.pos_next)
            return
        if with_head:
            hip._beam_candidates(cand, self.logits, self.eng.layout.Vpad, min(sh.V, 13317), self.seq, self.pos, sh.P, sh.msl + 2, temperature,
                                 rep, self.nb, self.cand_val, self.cand_id, self.B, **rules.tail(self.fixed_end))
        hip._beam_merge(merge, self.cand_val if with_head else None, self.cand_id if with_head else None, self.scores, self.seq, self.keep,
                        self.rows, self.pos, sh.P, sh.msl + 2, self.nb, self.n_prompts, self.pos_next, fixed_end=fe,
                        groups=rules.groups, diversity_penalty=rules.diversity_penalty)

    def _step_state(self):
        return super()._step_state() + [self.rows, self.scores]

    def _upload_keywords(self, tabs):
        """The keyword tables of a generation into this decoder's buffers, and the nb + K wide candidate tables as views of storage
        sized for the most keywords nb allows -- all allocated once: captured graphs hold their addresses (K is in the graph key).
        None without keywords."""
        if tabs is None:
            return None
        dev, B, nb = self.eng.dev, self.B, self.nb
        if self._kw_buf is None:
            sent, wmax = self.eng.sh.msl + 2, min(nb + 8, 256 // nb)
            none = (torch.full((min(self.eng.sh.V, 13317),), -1, dtype=torch.int16, device=dev),
                    torch.full((B, (self.max_len - 1) // sent + 1), -1, dtype=torch.int8, device=dev), False)
            self._kw_buf = (torch.zeros(self.n_prompts, 8, 4, dtype=torch.int32, device=dev),
                            torch.zeros(self.n_prompts, 8, dtype=torch.int8, device=dev),
                            (torch.zeros(B * wmax, dtype=torch.float32, device=dev), torch.zeros(B * wmax, dtype=torch.int32, device=dev),
                             torch.zeros(B * wmax, dtype=torch.int32, device=dev)), none)
        phrases, lens, store, _ = self._kw_buf
        phrases.copy_(torch.from_numpy(tabs.phrases))
        lens.copy_(torch.from_numpy(tabs.lens))
        W = nb + tabs.K
        self._kw_cand = tuple(t[:B * W].view(B, W) for t in store)
        return phrases, lens, tabs.K, tabs.cap

    @staticmethod
    def _keywords_alone(keywords, G):
        """Keywords share the beams among banks, groups among themselves: one allocation at a time."""
        if keywords is not None and G > 1:
            raise ValueError("keywords= and num_beam_groups > 1 both allocate the beams: ask for one of them")

    # Beam search keeps no token log-probabilities: the merge reorders the rows after the selection, and tok_lp would have to be
    # reordered with seq; beams are scored afterwards, through generate.score_sequences.  A search is deterministic: the truncation
    # stages of a draw and Mirostat (GreedyDecoder.begin) have nothing to act on.
    _REFUSED = (
        (("return_logprobs",), lambda return_logprobs: not return_logprobs,
         "beam search has no return_logprobs (the merge reorders rows after the selection); score the beams with generate.score_sequences"),
        (_WARP_NAMES, _no_warp,
         "a search draws nothing: min_p / typical_p / epsilon_cutoff / eta_cutoff shape the distribution a sampled generation draws from "
         "(GreedyDecoder / generate_samples), and no sampling runs inside a beam or contrastive search"),
        (_MIROSTAT_NAMES, _no_mirostat,
         "a search draws nothing: mirostat_tau / mirostat_eta steer the surprise of what a sampled generation draws (GreedyDecoder / "
         "generate_samples), and no sampling runs inside a beam or contrastive search"))

    @classmethod
    def _refuse(cls, **settings):
        """What this search does not take, refused with the reason (``_run_refusals`` over the class's table); returns the rest."""
        return _run_refusals(cls._REFUSED, settings)

    def describe(self):
        return "%d beams per prompt, " % self.nb + super().describe()

    @torch.no_grad()
    def begin(self, batch, length, temperature=1.0, repitition_penalty=1.0, prefix=None, no_repeat_ngram_size=0, line_lengths=None,
              line_end_ids=None, templates=None, rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, refrain_scheme=None,
              num_beam_groups=1, diversity_penalty=0.0, keywords=None, **settings):
        """GreedyDecoder.begin on every prompt replicated over its beams (encoder inputs, prompt prefill, the prefix, the line
        constraints, the templates and the rhyme scheme: one per prompt; every beam finds its leader's rhyme in its own history), the
        ancestry table as the identity and the beam scores at [0, -inf, ...] per prompt.  Scores only accumulate at the free positions
        after a prompt's prefix.  settings: whatever else GreedyDecoder.begin takes, through ``_refuse``: return_logprobs=True raises
        ValueError, and so do min_p / typical_p / epsilon_cutoff / eta_cutoff and mirostat_tau at anything but their defaults.

        num_beam_groups / diversity_penalty (``check_groups``; the rule's home is include/mmtg_hip.h): G > 1 splits a prompt's beams
        into G groups of s = num_beams / G rows, each started at [0, -inf, ...] and searched on its own; at every step that calls
        the head the merge (mmtg_decode_beam_merge_groups) serves the groups in order and lowers a candidate by the penalty per
        earlier group's beam that took the same content id at this step.  The penalty steers the choice only: the scores stay the
        unpenalised sums.  G = 1 (the default) runs exactly the launches, graphs and graph keys of a search without the argument.

        keywords (``check_keywords``; the rule's home is include/mmtg_hip.h): phrases of 1 .. 4 content ids the lyric should contain,
        each at a place of the model's choice -- one list for all prompts or one per prompt, shared by a prompt's beams.  Every step
        that calls the head then ends in mmtg_decode_beam_candidates_kw (each row also offers its unmet keywords' next ids, where no
        other rule bans them) and mmtg_decode_beam_merge_kw (the beams are shared among the banks: how much of the keywords a
        hypothesis holds).  The tables are uploaded here, once.  Best effort: a keyword no allowed column can hold stays unmet.
        With num_beam_groups > 1 it is a ValueError.  None runs exactly the launches, graphs and graph keys of a search without
        the argument.

        refrain_scheme (``check_refrain``): one scheme per prompt, shared by its beams; every beam copies from its own (reordered)
        history.  A copy is offered by the candidates the way a template's given id is (mmtg_decode_beam_candidates_refrain), so the
        merge and the scores are untouched -- and so every copy column still calls the head: head skipping is GreedyDecoder's, the
        known remainder here.  Beam groups need nothing.  keywords= together with a scheme is a ValueError: the one combination
        left out."""
        settings = BeamDecoder._refuse(**settings)
        for k in _DRAW_NAMES:       # (the base signature's sampling arguments: a beam search draws nothing and never read them)
            settings.pop(k, None)
        G, lam = check_groups(self.nb, num_beam_groups, diversity_penalty)
        self._keywords_alone(keywords, G)
        n = batch["img_embs"].shape[0]
        if n != self.n_prompts:
            raise ValueError("decoder was built for %d prompts, got %d" % (self.n_prompts, n))
        cons = _check_constraints(prefix, no_repeat_ngram_size, line_lengths, line_end_ids, n, length, self.eng.sh, "%d prompts" % n,
                                  templates, rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme)
        refrain_without_keywords(keywords, cons.lines)
        kw = check_keywords(keywords, n, self.nb, self.eng.sh.V, self.eng.sh.msl + 2, prefix=cons.prefix)
        cons = cons.repeat(self.nb)
        rep = {k: (v.repeat_interleave(self.nb, 0) if torch.is_tensor(v) else v) for k, v in batch.items()}
        n_steps = super().begin(rep, length, temperature, repitition_penalty, prefix=cons.prefix, no_repeat_ngram_size=cons.ngram,
                                line_lengths=cons.lines, _search={"groups": G, "diversity_penalty": lam, "kw": self._upload_keywords(kw)},
                                **settings)
        B, dev = self.B, self.eng.dev
        self.rows.copy_(torch.arange(B, dtype=torch.int32, device=dev)[:, None].expand(B, self.Tmax))
        sc = torch.full((n, self.nb), float("-inf"), dtype=torch.float32, device=dev)
        sc[:, ::self.nb // G] = 0.0                              # the first row of every group
        self.scores.copy_(sc.view(-1))
        return n_steps

    @torch.no_grad()
    def generate(self, batch, length, num_beam_groups=1, diversity_penalty=0.0, return_groups=False, keywords=None, return_met=False,
                 **settings):
        """batch: n = max_prompts prompts (GreedyDecoder.generate's keys); settings: temperature, repitition_penalty, use_graph and the
        constraints, as GreedyDecoder.generate takes them (``_refuse`` says what of the rest a search refuses).  Returns (ids [n, num_beams, 1 + length] in
        GreedyDecoder.generate's column layout, scores [n, num_beams] fp32), best first; ties go to the lower final row.
        prefix: one per prompt (check_prefix), shared by its beams.  no_repeat_ngram_size: as GreedyDecoder.generate, per beam
        on its own (reordered) history.  line_lengths / line_end_ids / templates: as GreedyDecoder.generate, one per prompt, shared by
        its beams (a given column adds nothing to a score).  rhyme_scheme / rhyme_classes / rhyme_distinct: as GreedyDecoder.generate,
        one scheme per prompt; each beam rhymes with its own earlier lines.  refrain_scheme: as GreedyDecoder.generate, one scheme per
        prompt; each beam repeats its own earlier line (not together with keywords: ValueError).  return_logprobs=True raises ValueError before any device
        work: the scores here are sums over the PROCESSED logits; generate.score_sequences gives a beam's raw log-probabilities.
        num_beam_groups / diversity_penalty: diverse beam search (``begin``): G groups of num_beams / G beams, a later group steered
        away from the ids earlier groups take at the same step.  The result keeps its form: all num_beams hypotheses of a prompt,
        best first by their (unpenalised) scores.  return_groups=True adds a third tensor, int64 [n, num_beams]: the group (final
        row // (num_beams / G)) of the hypothesis returned at that place.
        keywords: phrases the lyric should contain (``begin``, ``check_keywords``).  The hypotheses of a prompt are then ordered by
        (number of keywords met descending, score descending, stable); return_met=True adds an int64 [n, num_beams] tensor, that
        number for each hypothesis returned (``constraints.keywords_met`` of its ids).  Best effort: a keyword may stay unmet, and
        is reported so.  Not together with num_beam_groups > 1 or return_logprobs (ValueError).
        min_p / typical_p / epsilon_cutoff / eta_cutoff, mirostat_tau > 0: refused at anything but their defaults (ValueError): a
        search draws nothing."""
        settings = BeamDecoder._refuse(**settings)
        G, lam = check_groups(self.nb, num_beam_groups, diversity_penalty)
        self._keywords_alone(keywords, G)
        if return_met and keywords is None:
            raise ValueError("return_met reports the keywords a hypothesis holds: give keywords=")
        ids = super().generate(batch, length, num_beam_groups=G, diversity_penalty=lam, keywords=keywords, **settings)
        n, nb = self.n_prompts, self.nb
        ids = ids.view(n, nb, -1)
        sc = self.scores.view(n, nb).clone()
        order = torch.sort(sc, dim=1, descending=True, stable=True).indices
        if keywords is not None:            # (met descending, score descending, stable): a stable sort by met of the score order
            lists = check_keywords(keywords, n, nb, self.eng.sh.V, self.eng.sh.msl + 2).lists
            host = ids.cpu().tolist()
            met = torch.tensor([[keywords_met(host[p][r], lists[p]) for r in range(nb)] for p in range(n)], dtype=torch.long, device=sc.device)
            order = torch.gather(order, 1, torch.sort(torch.gather(met, 1, order), dim=1, descending=True, stable=True).indices)
            out = torch.gather(ids, 1, order[:, :, None].expand_as(ids)), torch.gather(sc, 1, order)
            return out + (torch.gather(met, 1, order),) if return_met else out
        out = torch.gather(ids, 1, order[:, :, None].expand_as(ids)), torch.gather(sc, 1, order)
        return out + (order // (nb // G),) if return_groups else out


class ContrastiveDecoder(BeamDecoder):
    """Contrastive search (Su et al. 2022; `penalty_alpha` / `top_k` of transformers' generate) on the beam decoder's machinery:
    `top_k` rows per prompt advance in lock step, and the token step ends in three launches -- the beam candidates the generation's
    rules name, unchanged; mmtg_decode_contrastive_sim; mmtg_decode_contrastive_merge (include/mmtg_hip.h states the rule).

    The newest column of a prompt's rows holds the model's k most probable tokens; the step runs the model on each, and the merge
    keeps the one with the best (1 - alpha) * p - alpha * s: p the processed probability the token was offered at, s the largest
    cosine between its last-layer hidden state (ln_f of the final residual stream, unit length) and those of the lyric so far.
    The context is the lyric alone, [#START#] / [#EOS#] columns included and PAD columns excluded; the prompt's topic words are not
    part of it (the batched prefill leaves no last-layer states for them, and the penalty is about the lyric repeating itself).
    One deterministic lyric per prompt, at about the cost of a k-beam search: no ban list, and every line rule composes, since the
    rules act in the candidates.  alpha = 0 is greedy decoding bit for bit at any k, and so is k = 1 at any alpha.

    The last column keeps its most probable candidate: no later step exists to judge it (at the usual lengths it is a forced
    [#EOS#]).  The score is the sum of the processed log-probabilities of the chosen tokens, a beam score's scale."""

    _prefill_prompt_only = True     # a prefix goes through token steps: every lyric column gets a hidden state

    def __init__(self, model, max_prompts, top_k, max_len=None, use_graph=True, lanes=1):
        k, _ = check_contrastive(top_k, 0.0)
        super().__init__(model, max_prompts, k, max_len=max_len, use_graph=use_graph, lanes=lanes)
        dev, D = self.eng.dev, self.eng.sh.D
        if D % 4 or D > 1024:
            raise ValueError("contrastive search holds n_embd up to 1024, a multiple of 4 (got %d)" % D)
        self.Hc = torch.zeros(self.B, self.max_len + 1, D, dtype=torch.float32, device=dev)     # unit ln_f states per lyric column
        self.sim = torch.zeros(self.B, dtype=torch.float32, device=dev)
        self.total = torch.zeros(self.n_prompts, dtype=torch.float32, device=dev)
        self.alpha = 0.0

    # What contrastive search does not take (the sampling arguments are the base classes', and would otherwise be ignored in silence)
    _REFUSED = BeamDecoder._REFUSED[1:] + (
        (("diversity_penalty",), lambda diversity_penalty: not diversity_penalty,
         "contrastive search has no diversity_penalty: there are no beam groups to keep apart"),
        (_DRAW_NAMES, _no_draw,
         "contrastive search is deterministic: it takes no sampling top_k / top_p / generator (its top_k is the decoder's, given at "
         "construction)"),
        (("keywords",), lambda keywords: keywords is None,
         "contrastive search takes no keywords=: it keeps one hypothesis per prompt, and a keyword needs banks of beams to be carried in "
         "(BeamDecoder / generate_beams)"),
        (("num_beam_groups",), lambda num_beam_groups: num_beam_groups == 1,
         "contrastive search has no num_beam_groups: its rows are one step's candidates, not beams to group"),
        (("return_logprobs",), lambda return_logprobs: not return_logprobs,
         "contrastive search has no return_logprobs (the merge reorders rows after the selection); score the lyric with "
         "generate.score_sequences"))

    def _select(self, with_head):
        """The step's last three launches: the candidates entry select_forms names (a step with the head), the similarity of every
        row's hidden state to its lyric context, the contrastive merge."""
        eng, sh, rules = self.eng, self.eng.sh, self.rules
        temperature, rep, _, _ = self.params
        fe = self.fixed_end if rules.prefix else None
        if with_head:
            hip._beam_candidates(rules.forms(with_head)[0], self.logits, eng.layout.Vpad, min(sh.V, 13317), self.seq, self.pos, sh.P,
                                 sh.msl + 2, temperature, rep, self.nb, self.cand_val, self.cand_id, self.B, **rules.tail(self.fixed_end))
        pre = "decoder.gpt2.transformer."
        # self.h: the residual stream the last block left, in every step variant (what the head's LayerNorm reads)
        hip.decode_contrastive_sim(self.h, eng.P(pre + "ln_f.weight"), eng.P(pre + "ln_f.bias"), sh.eps, self.Hc, self.sim, self.keep,
                                   self.rows, self.pos, sh.P, self.B, sh.D, scores=self.scores)
        hip.decode_contrastive_merge(self.cand_val if with_head else None, self.cand_id if with_head else None, self.scores, self.sim,
                                     self.total, self.alpha, self.seq, self.keep, self.rows, self.pos, sh.P, sh.msl + 2, self.nb,
                                     self.n_prompts, pos_next=self.pos_next, fixed_end=fe)

    def _graph_key(self, with_head, parity):
        return super()._graph_key(with_head, parity) + (("contrastive", self.alpha),)       # (alpha is captured by value)

    def _step_state(self):
        return super()._step_state() + [self.total]

    def describe(self):
        return "contrastive search, %d candidates per prompt, " % self.nb + GreedyDecoder.describe(self)

    @torch.no_grad()
    def begin(self, batch, length, penalty_alpha=0.6, **settings):
        """BeamDecoder.begin with the decoder's top_k rows per prompt, scores [0, -inf, ...] and total 0 per prompt.  settings:
        temperature, repitition_penalty and the constraints, as BeamDecoder.begin takes them.  With a prefix the prefill covers the prompt
        only, so every lyric column gets its hidden state from a token step; the steps at which every row is held skip the head.
        keywords=, num_beam_groups > 1, return_logprobs=True, a diversity penalty and sampling arguments (`top_k`, `top_p`, `generator`
        are the base signature's) are refused (ValueError, ``_refuse``) before any device work."""
        settings = ContrastiveDecoder._refuse(**settings)
        _, alpha = check_contrastive(self.nb, penalty_alpha)
        n_steps = super().begin(batch, length, **settings)
        self.alpha = alpha
        self.total.zero_()
        self.sim.zero_()
        if self.rules.prefix:       # (the prefill stopped at the prompt; columns every row holds still need no head)
            self.min_fixed = int(self.fixed_end.min().item())
        return n_steps

    @torch.no_grad()
    def generate(self, batch, length, penalty_alpha=0.6, **settings):
        """batch: n = max_prompts prompts (GreedyDecoder.generate's keys).  Returns (ids [n, 1 + length] in GreedyDecoder.generate's
        column layout, scores [n] fp32): one lyric per prompt and the sum of the processed log-probabilities of its chosen tokens.
        penalty_alpha in [0, 1]: the weight of the degeneration penalty (0: greedy decoding).  settings: temperature,
        repitition_penalty, use_graph, prefix, no_repeat_ngram_size, line_lengths / line_end_ids, templates, rhyme_scheme /
        rhyme_classes / rhyme_distinct, refrain_scheme: as BeamDecoder.generate, one per prompt.  What ``begin`` refuses raises
        ValueError."""
        settings = ContrastiveDecoder._refuse(**settings)
        ids = GreedyDecoder.generate(self, batch, length, penalty_alpha=penalty_alpha, **settings)
        n, k = self.n_prompts, self.nb
        return ids.view(n, k, -1)[:, 0].clone(), self.total + self.scores.view(n, k)[:, 0]


class StochasticBeamDecoder(BeamDecoder):
    """Stochastic beam search (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them") on the beam decoder's
    machinery: `num_samples` rows per prompt advance in lock step, and a token step that calls the head ends in
    mmtg_decode_gumbel_candidates and mmtg_decode_gumbel_merge (include/mmtg_hip.h states the rule; constraints.gumbel_candidates
    and gumbel_merge restate it).

    Every row keeps, beside its beam score, a perturbed value `gum`: its log-probability plus Gumbel noise, conditioned on its
    parent's.  The candidates offer a row's `num_samples` best perturbed children, the merge keeps the prompt's `num_samples` best
    overall.  The result is `num_samples` DIFFERENT lyrics per prompt, an exact sample without replacement from the distribution a
    sampled generation draws from -- the processed logits: penalty, temperature, bans and every line rule, which act in the
    candidates -- in the order they were drawn: row 0 is an ordinary sample (gum exactly 0), the later rows are what further draws
    would give were repeats thrown away.  One row is ancestral sampling by the Gumbel-max trick.  The noise is a counter-based hash
    of (the row's seed word, the position, the id), so a generation is a function of its seed and a replayed graph draws fresh
    noise at every step."""

    def __init__(self, model, max_prompts, num_samples, max_len=None, use_graph=True, lanes=1):
        nb, _ = check_stochastic(num_samples, 0)
        super().__init__(model, max_prompts, nb, max_len=max_len, use_graph=use_graph, lanes=lanes)
        dev, sent = self.eng.dev, self.eng.sh.msl + 2
        # allocated once: captured graphs hold their addresses
        self.gum = torch.zeros(self.B, dtype=torch.float32, device=dev)
        self.row_seed = torch.zeros(self.B, dtype=torch.int32, device=dev)         # (the library reads the words as uint32)
        self.cand_g = torch.zeros(self.B, nb, dtype=torch.float32, device=dev)
        self._no_src = torch.full((self.B, (self.max_len - 1) // sent + 1), -1, dtype=torch.int8, device=dev)      # "no copy line"

    # What stochastic beam search does not take
    _REFUSED = (
        (_WARP_NAMES, _no_warp,
         "stochastic beam search samples from the whole processed distribution: min_p / typical_p / epsilon_cutoff / eta_cutoff would "
         "truncate it before the perturbation, which is not built (a sampled generation takes them: GreedyDecoder / generate_samples)"),
        (_MIROSTAT_NAMES, _no_mirostat,
         "stochastic beam search has no mirostat_tau / mirostat_eta: Mirostat adapts a cut per row and draw, and the rows here are "
         "reordered by the merge (GreedyDecoder / generate_samples take it)"),
        (_DRAW_NAMES, _no_draw,
         "stochastic beam search takes no sampling top_k / top_p / generator: it samples from the whole processed distribution, and its "
         "noise comes from seed="),
        (("keywords",), lambda keywords: keywords is None,
         "stochastic beam search takes no keywords=: its rows are samples in draw order, not banks of beams to carry a keyword in "
         "(BeamDecoder / generate_beams)"),
        (("num_beam_groups", "diversity_penalty"), lambda num_beam_groups=1, diversity_penalty=0.0: num_beam_groups == 1 and not diversity_penalty,
         "stochastic beam search has no num_beam_groups / diversity_penalty: a penalty between groups would change the distribution the "
         "samples come from"),
        (("return_logprobs",), lambda return_logprobs: not return_logprobs,
         "stochastic beam search has no return_logprobs (the merge reorders rows after the selection); score the samples with "
         "generate.score_sequences"))

    def _select(self, with_head):
        """The step's last launches: on a step with the head the Gumbel candidates (one entry over the refrain form, whatever rules
        the generation has or none) and the Gumbel merge; otherwise the merge with null candidates."""
        eng, sh, rules = self.eng, self.eng.sh, self.rules
        temperature, rep, _, _ = self.params
        fe = self.fixed_end if rules.prefix else None
        if with_head:
            hip.decode_gumbel_candidates(self.logits, eng.layout.Vpad, min(sh.V, 13317), self.seq, self.pos, sh.P, sh.msl + 2, temperature,
                                         rep, self.nb, self.cand_val, self.cand_id, self.cand_g, self.scores, self.gum, self.row_seed,
                                         self.B, **rules.tail(self.fixed_end, "src", self._no_src))
        hip.decode_gumbel_merge(self.cand_val if with_head else None, self.cand_id if with_head else None,
                                self.cand_g if with_head else None, self.scores, self.gum, self.seq, self.keep, self.rows, self.pos, sh.P,
                                sh.msl + 2, self.nb, self.n_prompts, pos_next=self.pos_next, fixed_end=fe)

    def _graph_key(self, with_head, parity):
        # (on a head step: which of the refrain form's tables the launch holds, and a real src or none)
        return super()._graph_key(with_head, parity) + (("stochastic",) + (self.rules.src_key() if with_head else ()),)

    def _step_state(self):
        """BeamDecoder's state plus gum: without it the warm-up step of a graph capture would merge twice."""
        return super()._step_state() + [self.gum]

    def describe(self):
        return "stochastic beam search, %d samples per prompt, " % self.nb + GreedyDecoder.describe(self)

    @torch.no_grad()
    def begin(self, batch, length, seed=0, first_prompt=0, **settings):
        """BeamDecoder.begin with the decoder's num_samples rows per prompt, scores and gum at [0, -inf, ...] per prompt, and the rows'
        seed words written from `seed` (``stochastic_row_seeds``: a word per prompt and beam slot; `first_prompt` is the index of
        this batch's first prompt in the whole call, so that cutting a call into batches does not change a prompt's noise).
        settings: temperature, repitition_penalty and the constraints, as BeamDecoder.begin takes them.  keywords=,
        num_beam_groups > 1, a diversity penalty, return_logprobs=True, sampling top_k / top_p / generator, the four truncation stages
        and Mirostat are refused (ValueError, ``_refuse``) before any device work."""
        settings = StochasticBeamDecoder._refuse(**settings)
        _, seed = check_stochastic(self.nb, seed)
        n_steps = super().begin(batch, length, **settings)
        self.gum.copy_(self.scores)                             # [0, -inf, ...] per prompt
        words = stochastic_row_seeds(seed, first_prompt, self.n_prompts, self.nb)
        self.row_seed.copy_(torch.from_numpy(words.view(np.int32)))
        self.cand_g.fill_(float("-inf"))
        return n_steps

    @torch.no_grad()
    def generate(self, batch, length, seed=0, first_prompt=0, **settings):
        """batch: n = max_prompts prompts (GreedyDecoder.generate's keys).  Returns (ids [n, num_samples, 1 + length] in
        GreedyDecoder.generate's column layout, scores [n, num_samples] fp32, gum [n, num_samples] fp32) in draw order: the samples
        of a prompt are pairwise different, scores are the sums of the processed log-probabilities of their tokens (a beam score's
        scale), gum their perturbed values (0 for the first, then non-increasing).  A prompt whose rules leave fewer than
        num_samples different lyrics has dead rows at the end: score and gum -inf.  seed: an integer in 0 .. 2^32 - 1; equal seeds
        give equal bits.  settings: temperature, repitition_penalty, use_graph, prefix, no_repeat_ngram_size, line_lengths /
        line_end_ids, templates, rhyme_scheme / rhyme_classes / rhyme_distinct, refrain_scheme: as BeamDecoder.generate, one per
        prompt.  What ``begin`` refuses raises ValueError."""
        settings = StochasticBeamDecoder._refuse(**settings)
        ids = GreedyDecoder.generate(self, batch, length, seed=seed, first_prompt=first_prompt, **settings)
        n, nb = self.n_prompts, self.nb
        gum = self.gum.view(n, nb).clone()
        sc = torch.where(gum > float("-inf"), self.scores.view(n, nb), torch.full_like(gum, float("-inf")))
        return ids.view(n, nb, -1).clone(), sc, gum


class GuidedDecoder(GreedyDecoder):
    """Classifier-free guidance on the KV-cached, graph-replayed token step: how strongly the text follows its inputs.  Built for
    `max_prompts` = N prompts, the decoder runs 2 N rows: rows 0 .. N - 1 are the prompts, rows N .. 2 N - 1 their negatives (another
    prompt, or the same one without its images and texts: generate.without_experience).  Rows never interact, so the prompt prefill
    and the token step see 2 N ordinary rows; a step that calls the head then ends in

        mmtg_decode_guidance   glogits[b] = lu + s * (lc - lu) over the log-softmax of the raw logits rows b and N + b, b < N
        the selection entry a plain decoder would pick, over N rows, reading glogits -- penalty, temperature, bans, every
            constraint, top-k / top-p, the four cuts and Mirostat all act on the guided scores
        mmtg_decode_logprob    (with return_logprobs) over the N raw prompt rows: the log-probability stays the model's own
        mmtg_decode_mirror     seq[N + b, pos + 1] = seq[b, pos + 1]: the negatives stay on the prompts' text

    and a step without the head in the selection it always ended in, over N rows, and the mirror.  Only the first N rows of the
    constraint tables, the uniforms, ``mirostat_mu`` and ``tok_lp`` are ever read or written by a selection.  The guided scores are
    log-probabilities, never positive, where raw logits have either sign, and the per-occurrence repetition penalty (a division,
    whatever the sign: generate.py:127-131) acts on the number it finds: guidance_scale = 1 with a penalty is not the plain decoder
    (without one it is, up to rounding: log-softmax keeps the order).  One lane (the halves must meet in one launch)."""

    def __init__(self, model, max_prompts, max_len=None, use_graph=True, lanes=1):
        if lanes != 1:
            raise ValueError("guided decoding runs on one lane (got lanes=%r)" % (lanes,))
        n = int(max_prompts)
        if n < 1:
            raise ValueError("max_prompts %r must be at least 1" % (max_prompts,))
        super().__init__(model, 2 * n, max_len=max_len, use_graph=use_graph, lanes=1)
        self.n_prompts = n
        self.guidance_scale = GUIDANCE_OFF
        # the guided scores, allocated once: captured graphs hold the address.  Columns V .. Vpad - 1 are never written nor read.
        self.glogits = torch.zeros(n, self.eng.layout.Vpad, dtype=torch.float32, device=self.eng.dev)
        # what GreedyDecoder._select / _logprob read in place of the step's own logits and row count
        self.select_rows, self.select_logits = n, self.glogits

    def _select(self, with_head):
        if with_head:
            hip.decode_guidance(self.logits, self.logits[self.n_prompts:], self.eng.layout.Vpad, min(self.eng.sh.V, 13317),
                                self.guidance_scale, self.glogits, self.n_prompts)
        super()._select(with_head)

    def _end_step(self, with_head):
        hip.decode_mirror(self.seq, self.pos, self.n_prompts)      # the step's last launch; it reads the slot the selection left alone

    def _begin_lead(self, batch, length):
        return (batch,) + self._negative_and_scale[:1] + (length,) + self._negative_and_scale[1:]

    def _result_rows(self):
        return self.n_prompts

    def _graph_key(self, with_head, parity):
        return super()._graph_key(with_head, parity) + (("guidance", self.guidance_scale),)

    def describe(self):
        return super().describe() + ", %d prompts beside their negatives (guidance_scale %g)" % (self.n_prompts, self.guidance_scale)

    @torch.no_grad()
    def begin(self, batch, negative_batch, length, guidance_scale=GUIDANCE_OFF, temperature=1.0, repitition_penalty=1.0, top_k=1, top_p=0.0,
              generator=None, prefix=None, no_repeat_ngram_size=0, line_lengths=None, line_end_ids=None, templates=None,
              rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, return_logprobs=False, keywords=None, refrain_scheme=None,
              **sampler_kw):
        """GreedyDecoder.begin for N prompts (batch) and their N negatives (negative_batch, the same keys): the two are concatenated,
        the constraints and prefixes -- one per prompt -- are doubled, and guidance_scale (check_guidance) is kept for the steps.
        sampler_kw: min_p / typical_p / epsilon_cutoff / eta_cutoff / mirostat_tau / mirostat_eta, as GreedyDecoder.begin takes them."""
        _keywords_need_beams(keywords)
        scale = check_guidance(guidance_scale)
        n, sh = self.n_prompts, self.eng.sh
        for name, b in (("batch", batch), ("negative_batch", negative_batch)):
            if b["img_embs"].shape[0] != n:
                raise ValueError("decoder was built for %d prompts, %s has %d" % (n, name, b["img_embs"].shape[0]))
        dev = self.eng.dev
        # (an input the negative does not name is the prompt's own: a negative differs in what it is given to differ in)
        both = {k: torch.cat([torch.as_tensor(batch[k]).to(dev), torch.as_tensor(negative_batch.get(k, batch[k])).to(dev)]) for k in batch
                if k not in ("targets", "rating")}
        cons = _check_constraints(prefix, no_repeat_ngram_size, line_lengths, line_end_ids, n, length, sh, "%d prompts" % n, templates,
                                  rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme).take(list(range(n)) * 2)
        self.guidance_scale = scale
        return super().begin(both, length, temperature, repitition_penalty, top_k, top_p, generator, prefix=cons.prefix,
                             no_repeat_ngram_size=cons.ngram, line_lengths=cons.lines, return_logprobs=return_logprobs, **sampler_kw)

    @torch.no_grad()
    def generate(self, batch, negative_batch, length, guidance_scale=GUIDANCE_OFF, **kw):
        """batch / negative_batch: N prompts and their N negatives (GreedyDecoder.generate's keys).  Returns the prompts' lyric ids
        [N, 1 + length] -- with return_logprobs (ids, tok_lp [N, 1 + length]), the log-probability the RAW logits of the prompt's own
        row give each id.  guidance_scale: 0 follows the negative alone, 1 the prompt alone, more sharpens the prompt against the
        negative.  kw: everything else GreedyDecoder.generate takes but `teacher` (temperature, repitition_penalty, top_k, top_p,
        generator, use_graph, tap, prefix, the constraints, the samplers, return_logprobs), one per prompt.  `tap(j, with_head, picked
        [2 N], logits [2 N, Vpad] or None)` receives the raw logits of both halves.  The loop is GreedyDecoder.generate's own."""
        if kw.get("teacher") is not None:
            raise ValueError("guided decoding takes no teacher: the two halves of the batch follow one text, the prompts' own")
        self._negative_and_scale = (negative_batch, guidance_scale)
        try:
            return super().generate(batch, length, **kw)
        finally:
            self._negative_and_scale = None


class ModalityGuidedDecoder(GuidedDecoder):
    """Per-modality guidance on the KV-cached, graph-replayed token step: a scale for the experience as a whole, one for the images and
    one for the texts.  Built for `max_prompts` = N prompts and `blocks` = K (3 or 4; 2 works and is GuidedDecoder's case through the
    K-row kernels), the decoder runs K N rows: block 0 (rows 0 .. N - 1) holds the prompts, block k the k-th running negative of the
    same prompts, in the fixed branch order u (generate.without_experience), i (without_images), t (without_texts) -- a branch runs
    only if its scale differs from 1.  Rows never interact, so the prefill and the token step see K N ordinary rows; a step that calls
    the head then ends in

        mmtg_decode_guidance_multi   glogits[b] = lc + sum_k (s_k - 1) (lc - l_k) over the log-softmax of the raw logits rows k N + b
        the selection entry a plain decoder would pick, over N rows, reading glogits
        mmtg_decode_logprob          (with return_logprobs) over the N raw prompt rows
        mmtg_decode_mirror_multi     seq[k N + b, pos + 1] = seq[b, pos + 1], k = 1 .. K - 1: every block stays on the prompts' text

    and a step without the head in its selection over N rows and the mirror.  The scales are host numbers handed to the kernel by
    value at capture, so the graph key carries the branch set and the scales: other scales capture other graphs.  Everything else is
    GuidedDecoder's: the constraint tables, the uniforms, ``mirostat_mu`` and ``tok_lp`` are touched for the first N rows only, the
    log-probabilities stay the model's own, one lane."""

    def __init__(self, model, max_prompts, blocks, max_len=None, use_graph=True, lanes=1):
        if lanes != 1:
            raise ValueError("guided decoding runs on one lane (got lanes=%r)" % (lanes,))
        n, k = int(max_prompts), int(blocks)
        if n < 1:
            raise ValueError("max_prompts %r must be at least 1" % (max_prompts,))
        if not 2 <= k <= 4:
            raise ValueError("blocks %r must be 2, 3 or 4: a prompt beside one to three negatives" % (blocks,))
        GreedyDecoder.__init__(self, model, k * n, max_len=max_len, use_graph=use_graph, lanes=1)
        self.n_prompts, self.blocks = n, k
        self.guidance_scale = GUIDANCE_OFF      # (GuidedDecoder's attribute; the u branch's scale when it runs)
        self.branches, self.scales = (), ()
        self.glogits = torch.zeros(n, self.eng.layout.Vpad, dtype=torch.float32, device=self.eng.dev)
        self.select_rows, self.select_logits = n, self.glogits

    def _select(self, with_head):
        if with_head:
            hip.decode_guidance_multi(self.logits, self.eng.layout.Vpad, min(self.eng.sh.V, 13317), self.scales, self.glogits,
                                      self.n_prompts)
        GreedyDecoder._select(self, with_head)

    def _end_step(self, with_head):
        hip.decode_mirror_multi(self.seq, self.pos, self.n_prompts, self.blocks)

    def _graph_key(self, with_head, parity):
        return GreedyDecoder._graph_key(self, with_head, parity) + (("modality_guidance", self.branches, self.scales),)

    def describe(self):
        return GreedyDecoder.describe(self) + ", %d prompts beside %d negatives each (%s)" % (
            self.n_prompts, self.blocks - 1, ", ".join("%s %g" % bs for bs in zip(self.branches, self.scales)))

    @torch.no_grad()
    def begin(self, batch, negative_batches, length, branches=(), scales=(), temperature=1.0, repitition_penalty=1.0, top_k=1, top_p=0.0,
              generator=None, prefix=None, no_repeat_ngram_size=0, line_lengths=None, line_end_ids=None, templates=None,
              rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, return_logprobs=False, keywords=None, refrain_scheme=None,
              **sampler_kw):
        """GreedyDecoder.begin for N prompts (batch) and their K - 1 negatives (negative_batches: a list of K - 1 batches with the same
        keys, in branch order): the K are concatenated, the constraints and prefixes -- one per prompt -- are repeated K times, and
        the branch names (for the graph key and ``describe``) and their scales (each as check_guidance takes it) are kept for the steps."""
        _keywords_need_beams(keywords)
        scales = tuple(check_guidance(s) for s in scales)
        branches = tuple(str(b) for b in branches)
        n, k, sh = self.n_prompts, self.blocks, self.eng.sh
        if len(negative_batches) != k - 1 or len(scales) != k - 1 or len(branches) != k - 1:
            raise ValueError("decoder was built for %d negatives per prompt, got %d batches, %d branches and %d scales"
                             % (k - 1, len(negative_batches), len(branches), len(scales)))
        for name, b in [("batch", batch)] + [("negative_batches[%d]" % i, nb) for i, nb in enumerate(negative_batches)]:
            if b["img_embs"].shape[0] != n:
                raise ValueError("decoder was built for %d prompts, %s has %d" % (n, name, b["img_embs"].shape[0]))
        dev = self.eng.dev
        every = {key: torch.cat([torch.as_tensor(batch[key]).to(dev)] + [torch.as_tensor(nb.get(key, batch[key])).to(dev)
                                                                         for nb in negative_batches])
                 for key in batch if key not in ("targets", "rating")}
        cons = _check_constraints(prefix, no_repeat_ngram_size, line_lengths, line_end_ids, n, length, sh, "%d prompts" % n, templates,
                                  rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme).take(list(range(n)) * k)
        self.branches, self.scales = branches, scales
        self.guidance_scale = dict(zip(branches, scales)).get("u", GUIDANCE_OFF)
        return GreedyDecoder.begin(self, every, length, temperature, repitition_penalty, top_k, top_p, generator, prefix=cons.prefix,
                                   no_repeat_ngram_size=cons.ngram, line_lengths=cons.lines, return_logprobs=return_logprobs, **sampler_kw)

    @torch.no_grad()
    def generate(self, batch, negative_batches, length, branches=(), scales=(), **kw):
        """batch: N prompts; negative_batches: their K - 1 negatives in branch order; branches / scales: the K - 1 branch names and
        scales (constraints.check_modality_guidance returns both).  Returns what GuidedDecoder.generate returns, for the prompts.
        kw: as GuidedDecoder.generate; `tap(j, with_head, picked [K N], logits [K N, Vpad] or None)` receives the raw logits of all K
        blocks."""
        if kw.get("teacher") is not None:
            raise ValueError("guided decoding takes no teacher: every block of the batch follows one text, the prompts' own")
        self._negative_and_scale = (list(negative_batches), tuple(branches), tuple(scales))
        try:
            return GreedyDecoder.generate(self, batch, length, **kw)
        finally:
            self._negative_and_scale = None
