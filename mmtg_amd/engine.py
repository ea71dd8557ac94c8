"""Explicit forward/backward engine of the MMTG hot path on MI355X.

No autograd, no tracing compiler: the training step is a fixed sequence of
C-ABI kernel launches (mmtg_amd.hip) over caller-owned HBM buffers.  The
forward keeps the activations the backward needs (288 GB of HBM3E: nothing is
recomputed except attention probabilities), the backward walks the layers in
reverse and deposits parameter gradients into ONE flat fp32 buffer whose
element order is the order in which gradients become final -- so contiguous
slices of it are the all-reduce buckets of the data-parallel path
(mmtg_amd.ddp) and can be launched while the backward is still running.

Reference semantics (file:line into /root/reference/src):
  MMTG.forward model.py:356-400, GPT2_Decoder.forward :225-327, the GPT-2
  arithmetic of transformers 4.12.3 behind model.py:282-288, MyLoss
  loss.py:45-74.  The oracle (oracle/mmtg_oracle.py) restates the same maths
  and is what the tests compare this engine against.
"""
from __future__ import annotations

import contextlib
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import hip
from .configs import rnn_param_shapes

ALIGN = 64  # elements; keeps every pack 16-byte aligned in both f32 and bf16


# --------------------------------------------------------------------------
# flat parameter layout
# --------------------------------------------------------------------------
class ParamLayout:
    """Flat layout of all parameters in gradient-ready order.

    ``packs`` are contiguous runs (no inner padding) so that e.g. the three
    alpha-attention projections form one [3H, H] GEMM operand."""

    def __init__(self, model_cfgs, gpt2_cfg):
        S = model_cfgs["seq_len"]
        E = model_cfgs["topic"]["input_dim"]
        H = model_cfgs["topic"]["hidden_dim"]
        D = gpt2_cfg["n_embd"]
        V = gpt2_cfg["vocab_size"]
        NP = gpt2_cfg["n_positions"]
        L = gpt2_cfg["n_layer"]
        self.Vpad = (V + 127) // 128 * 128
        pre = "decoder.gpt2.transformer."
        packs = []  # (pack_name, [(key, shape)], pad_tail_elems)
        packs.append(("ln_f.w", [(pre + "ln_f.weight", (D,))], 0))
        packs.append(("ln_f.b", [(pre + "ln_f.bias", (D,))], 0))
        self.layer_first_pack = {}
        for l in range(L - 1, -1, -1):
            p = f"{pre}h.{l}."
            self.layer_first_pack[l] = len(packs)
            for nm, shp in (("mlp.c_proj.weight", (4 * D, D)), ("mlp.c_proj.bias", (D,)),
                            ("mlp.c_fc.weight", (D, 4 * D)), ("mlp.c_fc.bias", (4 * D,)),
                            ("ln_2.weight", (D,)), ("ln_2.bias", (D,)),
                            ("attn.c_proj.weight", (D, D)), ("attn.c_proj.bias", (D,)),
                            ("attn.c_attn.weight", (D, 3 * D)), ("attn.c_attn.bias", (3 * D,)),
                            ("ln_1.weight", (D,)), ("ln_1.bias", (D,))):
                packs.append((p + nm, [(p + nm, shp)], 0))
        packs.append(("wte", [(pre + "wte.weight", (V, D))], (self.Vpad - V) * D))
        packs.append(("wpe", [(pre + "wpe.weight", (NP, D))], 0))
        for nm, shp in (("decoder.projector_layer2.weight", (D, H)), ("decoder.projector_layer2.bias", (D,)),
                        ("decoder.projector_layer1.weight", (H, E)), ("decoder.projector_layer1.bias", (H,)),
                        ("mm_atten_layer.out_linear.weight", (E, H)), ("mm_atten_layer.out_linear.bias", (E,))):
            packs.append((nm, [(nm, shp)], 0))
        packs.append(("att_w", [(f"mm_atten_layer.att_matrices.{i}.weight", (1, H)) for i in range(S)], 0))
        packs.append(("att_b", [(f"mm_atten_layer.att_matrices.{i}.bias", (1,)) for i in range(S)], 0))
        for mod in ("text", "img"):
            m = f"{mod}_inner_atten_layer."
            packs.append((mod + "_qkv_w", [(m + n + ".weight", (H, H)) for n in ("query", "key", "value")], 0))
            packs.append((mod + "_qkv_b", [(m + n + ".bias", (H,)) for n in ("query", "key", "value")], 0))
        for i in (3, 2, 1):
            packs.append((f"ln_layer{i}.weight", [(f"ln_layer{i}.weight", (H,))], 0))
            packs.append((f"ln_layer{i}.bias", [(f"ln_layer{i}.bias", (H,))], 0))
        for ch in ("text", "image"):
            r = f"encoder.rnns_{ch}."
            for layer in reversed(rnn_param_shapes(model_cfgs, ch)):     # the top layer's gradients are ready first
                for nm, shp in layer:
                    packs.append((r + nm, [(r + nm, shp)], 0))
        packs.append(("encoder.topic_fc.weight", [("encoder.topic_fc.weight", (H, E))], 0))
        packs.append(("encoder.topic_fc.bias", [("encoder.topic_fc.bias", (H,))], 0))

        self.entries = {}      # key -> (offset, shape, numel)
        self.pack_range = {}   # pack name -> (offset, numel incl. tail pad)
        self.pack_order = []
        off = 0
        for name, members, tail in packs:
            off = (off + ALIGN - 1) // ALIGN * ALIGN
            start = off
            for key, shape in members:
                n = int(np.prod(shape))
                self.entries[key] = (off, tuple(shape), n)
                off += n
            off += tail
            self.pack_range[name] = (start, off - start)
            self.pack_order.append(name)
        self.total = (off + ALIGN - 1) // ALIGN * ALIGN
        self.keys = [k for _, members, _ in packs for k, _ in members]

    def view(self, flat, key):
        off, shape, n = self.entries[key]
        return flat[off:off + n].view(shape)

    def pack(self, flat, name):
        off, n = self.pack_range[name]
        return flat[off:off + n]

    def buckets(self, bucket_elems, split_after=()):
        """Contiguous [start, end) ranges of ~bucket_elems elements on pack boundaries,
        in gradient-ready order.  `split_after`: pack names after which a bucket ends whatever its size -- the points of the
        backward's TAIL at which a run of gradients is final (the tied embedding + wpe once the input-embedding backward has
        run, the projector / fuser after the fuser's backward): what is left for the exchange after the last kernel is then
        the encoder's gradients only, not everything since the last full bucket."""
        out, start = [], 0
        forced = set(split_after)
        for name in self.pack_order:
            o, n = self.pack_range[name]
            end = o + n
            if end - start >= bucket_elems or (name in forced and end > start):
                out.append((start, end))
                start = end
        if start < self.total:
            out.append((start, self.total))
        return out


class Shapes:
    def __init__(self, model_cfgs, data_cfg, gpt2_cfg):
        self.S = model_cfgs["seq_len"]
        self.E = model_cfgs["topic"]["input_dim"]
        self.H = model_cfgs["topic"]["hidden_dim"]
        self.heads = model_cfgs["SELF_ATT"]["attention_heads"]
        self.P = data_cfg["topic_prompt_length"]
        self.msl = data_cfg["max_sent_length"]
        self.max_seq_length = data_cfg["max_seq_length"]
        self.two_sents = 2 * (self.msl + 2)
        self.D = gpt2_cfg["n_embd"]
        self.nH = gpt2_cfg["n_head"]
        self.L = gpt2_cfg["n_layer"]
        self.V = gpt2_cfg["vocab_size"]
        self.NP = gpt2_cfg["n_positions"]
        self.eps = gpt2_cfg.get("layer_norm_epsilon", 1e-5)
        self.pdrop = (gpt2_cfg.get("embd_pdrop", 0.1), gpt2_cfg.get("attn_pdrop", 0.1), gpt2_cfg.get("resid_pdrop", 0.1))
        # encoder channels (model.py:39-59): cell type, layers; dropout between the layers of a channel in training (nn.RNNBase)
        self.rnn = {ch: (model_cfgs[ch]["type"], int(model_cfgs[ch]["num_layers"])) for ch in ("image", "text")}
        self.rnn_pdrop = float(model_cfgs.get("dropout", 0.0))
        for ch in ("image", "text"):
            rnn_param_shapes(model_cfgs, ch)         # validates type / num_layers
            if model_cfgs[ch]["input_dim"] != self.E or model_cfgs[ch]["hidden_dim"] != self.H:
                raise ValueError("The hidden dim of topic, image and text must be equal (model.py:36); this engine also takes one input dim")
        if self.D % self.nH or self.D // self.nH != 64:
            raise ValueError("the attention kernels are built for head dim 64 (n_embd=%d, n_head=%d)" % (self.D, self.nH))
        if model_cfgs["MM_ATT"]["attention_dim"] != 1:
            raise ValueError("MM_ATT.attention_dim must be 1 (the reference's broadcast at model.py:200 requires it)")


def gaussian_prior(S):
    """q_i[j] ~ N(j; i, 1) normalised over j < S (model.py:116-120, 5 generalised to S)."""
    j = np.arange(S, dtype=np.float64)
    rows = []
    for i in range(S):
        v = np.exp(-0.5 * (j - i) ** 2) / math.sqrt(2 * math.pi)
        v32 = v.astype(np.float64)
        rows.append((v32 / v32.sum()).astype(np.float32))
    return np.stack(rows)


import os as _os


def _dist_rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else int(_os.environ.get("RANK", "0"))


_NO_OCC4 = bool(_os.environ.get("MMTG_GEMM_NO_OCC4"))     # A/B switch, mirrors the library's


def _wgrad_splits(M, N, K, occ4=False, slots=512, t_iter=1.1, t_fixed=6.0):
    """Split-K factor of a weight-gradient GEMM (K = tokens).  The 128x128-tile kernel keeps two
    workgroups per CU (512 slots on 256 CUs); a grid of tiles*s workgroups runs in
    ceil(tiles*s/512) rounds of (K/(64 s)) K-iterations each.  Pick the s with the smallest
    estimate -- e.g. 144 tiles: s=3 (432 WGs, one round) beats s=4 (576 WGs, two rounds) by 30 %
    on the GPU (profiles/r01_gemm_tn_split_sweep.log)."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if occ4 and not _NO_OCC4:
        # bf16: the single-stage kernel keeps FOUR workgroups per CU (1024 slots) and is throughput-bound,
        # so only the fill of the last round and the atomic volume matter.  Measured optima
        # (profiles/r01_v6_gemm_tn_split_sweep.log): 144 tiles -> 5, 108 -> 6..7, 630 -> 4, 36 -> 8+.
        smax = max(1, K // 256)
        s = round(760.0 / tiles) if tiles < 512 else round(2520.0 / tiles)
        return int(max(1, min(smax, s, 12)))
    best, best_t = 1, None
    for s in range(1, 33):
        if s > 1 and K // s < 256:
            break
        rounds = -(-tiles * s // slots)
        # + the fp32 atomic epilogue: 64 KB of adds per workgroup at the chip-wide ~1.3 TB/s atomic rate
        t = rounds * (K / (64.0 * s) * t_iter + t_fixed) + tiles * s * 65536 / 1.3e6
        if best_t is None or t < best_t * 0.97:
            best, best_t = s, t
    return best


_WGRAD_GROUP_SPLITS = int(_os.environ.get("MMTG_WGRAD_GROUP_SPLITS", "0"))    # 0 = the one-round rule below
# the bf16 decoder backward's small ordered column sums (LayerNorm second stages, dGELU bands, attention bias rows: 4 per block) summed
# by ONE batched launch per data-parallel hand-over point -- one per step without a bucket hook -- instead of a launch each (A/B switch)
_DEFER_SUMS = _os.environ.get("MMTG_DEFER_SUMS", "1") != "0"
# the grouped weight gradients of the LAST blocks the backward walks (blocks MMTG_WGRAD_TAIL - 1 .. 0) on a side stream beside the
# backward's tail -- the fuser / encoder backward: ~60 small dependent launches during which the GPU is mostly idle -- instead of inside
# the block loop; joined before the gradient norm.  Single-GPU steps with dropout on (their operands are the masked copies, which get
# buffers of their own: 209 MB per block at GPT-2 base); 0 = off.  Measured (same box, ms per step): 0: 14.91, 1-2: 14.9-15.0 (the
# co-running launches slow the tail as much as they hide), 4: 14.72, 6: 14.66, 8: 14.64, 12: 14.67; the same launches at the same
# place on the MAIN stream: 14.98 -- the gain is the overlap, not the order.  bf16x3 (plane-pair operands, with or without dropout):
# 33.57 -> 33.07 at 8 (33.03 at 4, 33.29 at 12)
_WGRAD_TAIL = int(_os.environ.get("MMTG_WGRAD_TAIL", "8"))
_LMHEAD_GROUP_SPLITS = int(_os.environ.get("MMTG_LMHEAD_GROUP_SPLITS", "0"))
# the grouped weight-gradient launches on a SIDE stream, one block behind the dgrad chain (MMTG_WGRAD_STREAM; see Engine._bwd_blocks)
_WGRAD_STREAM = _os.environ.get("MMTG_WGRAD_STREAM", "0") != "0"
# x3 grouped weight gradients: mmtg_wgrad_group's config 6 = combined stages (all four planes of a K tile per 64 KB stage, two
# workgroups per CU: 512 slots)
_X3_WG_CFG = 6
# 0: 128x128 tiles, four workgroups per CU; 1: 256x256 eight-phase; 2: 256x256, one 16-wave workgroup per CU over a 3-deep ring of
# 32-k stages (mmtg_wgrad_group's config 8 -- its 2 is the split-precision form).  Default 2: 14.71 -> 14.07 ms per step over three
# alternating pairs, the launch 275 -> 228 us, parameters and gradients bit-equal to config 0's (docs/experiments.md, last section)
_WGRAD_GROUP_CFG = int(_os.environ.get("MMTG_WGRAD_GROUP_CFG", "2"))


def _group_cfg(D, x3=False):
    """mmtg_wgrad_group configuration of the bf16 grouped launches (256x256 tiles need D >= 256 to fill them)."""
    if x3 or D < 256 or _WGRAD_GROUP_CFG not in (1, 2):
        return 0
    return hip.WGRAD_RING if _WGRAD_GROUP_CFG == 2 else 1


def _group_splits(tiles, K, slots=1024):
    """K splits of a grouped weight-gradient launch: tiles x splits workgroups in ONE round of the kernel's slots (four
    128x128 workgroups per CU / one 256x256 workgroup per CU), no K slice shorter than 1024 tokens."""
    if _WGRAD_GROUP_SPLITS > 0:
        return _WGRAD_GROUP_SPLITS
    return int(max(1, min(slots // max(1, tiles), K // 1024, 16)))


def _group_sizing(shapes, cfg, rule):
    """(K splits, workspace floats, counters) of a grouped launch over problems of the given (M, N) shapes in the kernel's tile
    configuration `cfg` (hip.wgrad_group_sizes'); rule(tiles) gives the split count.  No device access."""
    tiles = hip.wgrad_group_sizes(shapes, 1, cfg)[0]
    splits = rule(tiles)
    _, nws, ncnt = hip.wgrad_group_sizes(shapes, splits, cfg)
    return splits, nws, ncnt


def _group_splits_x3(tiles, K):
    """K splits of a split-precision grouped launch.  Combined stages (config 6, two workgroups per CU = 512 slots), measured at
    K = 15104 (tools/bench_wgrad_x3.py): one full round when the tiles fit (projector: 88 tiles x 5 = 122 us against 172 at x 6),
    else about four rounds' worth (tied embedding, 630 tiles: x 3 = 783 us, x 2 = 845, x 1 = 1054); a block's 432 tiles run within
    2 % of their best at any count from 1 to 5."""
    if _WGRAD_GROUP_SPLITS > 0:
        return _WGRAD_GROUP_SPLITS
    s = 512 // max(1, tiles)
    if s == 0:
        s = 2048 // tiles
    return int(max(1, min(s, K // 1024, 16)))


def _round_capacity(n):
    """Next value of {1, 1.25, 1.5, 1.75} x 2^k at or above n (<= 25 % slack, O(log) distinct sizes per buffer so the
    caching allocator's freed blocks are reused instead of piling up)."""
    if n <= 1024:
        return 1024
    k = 1 << (int(n - 1).bit_length() - 1)      # largest power of two below n
    for q in (4, 5, 6, 7, 8):
        if k * q // 4 >= n:
            return k * q // 4
    return 2 * k


def mix_seed(seed, site):
    """32-bit hash of (step seed, dropout site): sites get unrelated counter-hash streams instead of one stream
    at small integer offsets (the kernels compute hash(element index * G + seed))."""
    x = (seed ^ (0x9E3779B9 * (site + 1))) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 0x846CA68B) & 0xFFFFFFFF
    return (x ^ (x >> 16)) & 0xFFFFFFFF


EXP_DROP_SITE = 0x2000     # the experience dropout's site: the RNN layers use 0x1000 + 64 site + l (< 0x1100), the blocks 3 l + 1 .. 3


def initial_drop_seed(rank=0):
    """Start of the dropout counter: a hash of torch's seed (train.py:88-94 seeds torch) and the data-parallel rank,
    so replicas draw independent masks (the reference's DataParallel replicas do) and torch.manual_seed controls
    the sequence."""
    return mix_seed(torch.initial_seed() & 0xFFFFFFFF, 0x5EED + 7919 * rank)


# --------------------------------------------------------------------------
class Engine:
    """Owns the flat buffers and runs forward / loss / backward / optimizer."""

    def __init__(self, model_cfgs, data_cfg, gpt2_cfg, master, table, dtype=hip.BF16, x3=False, hybrid=False):
        hip.lib()  # fail loudly if the extension is not built
        if x3 and dtype != hip.F32:
            raise ValueError("the split-precision (bf16x3) products belong to fp32 storage")
        if hybrid and not x3:
            raise ValueError("the hybrid mode (bf16x3f) is the split-precision forward with a bf16 backward: it needs x3")
        if not master.is_cuda:
            raise RuntimeError("the MMTG engine runs on an MI355X (cuda) device only -- there is no CPU path")
        self.sh = Shapes(model_cfgs, data_cfg, gpt2_cfg)
        if x3 and self.sh.D % 128:
            # the split-precision products walk whole 128-wide K tiles of n_embd; an x3 engine has no mixed fallback for its training
            # step (its weight copies are plane pairs, its saved activations too), so a width it cannot serve is refused up front
            raise ValueError("compute_dtype='bf16x3' needs n_embd to be a multiple of 128 (got %d): use compute_dtype='f32'" % self.sh.D)
        self.layout = ParamLayout(model_cfgs, gpt2_cfg)
        assert master.numel() == self.layout.total and master.dtype == torch.float32
        self.dev = master.device
        self.dtype = dtype
        self.tdt = hip.torch_dtype(dtype)
        self.master = master
        self.grad = None
        self.wc = master if dtype == hip.F32 else torch.zeros(self.layout.total, device=self.dev, dtype=torch.bfloat16)
        # x3 (round 5): fp32 storage everywhere, the GPT-2 / LM-head products on the bf16 matrix cores as three passes over
        # (hi | lo) bf16 plane pairs (hip.gemm_x3).  wc2 = the plane pair of the whole flat parameter buffer.
        self.x3 = bool(x3)
        # hybrid ("bf16x3f", round 6): the forward of the x3 mode -- logits / loss / KL at the fp32 mode's parity -- and the backward of
        # the bf16 mode, ONE matrix-core pass per product, over the hi planes the forward stored (hi = bf16(x): exactly the tensor the
        # bf16 kernels take, same leading dimension) and the hi planes of the weights; the encoder / fuser stay exact fp32 both ways
        self.hybrid = bool(hybrid)
        self.wc2 = torch.zeros(2, self.layout.total, device=self.dev, dtype=torch.bfloat16) if self.x3 else None
        self.copies_fresh = dtype == hip.F32 and not self.x3
        self._init_transposed()
        self.set_table(table)
        self.prior = torch.from_numpy(gaussian_prior(self.sh.S)).to(self.dev)
        self.ws = {}
        self.act = None
        self.training = False
        self.drop_seed = initial_drop_seed(_dist_rank())
        self.wgrad_overwrite = False   # set by MMTGTrainer.step around its backward
        self._ow_desc, self._ow_rec = {}, None   # zero lists per step shape / the record in progress (zero_grad)
        self._lazy = None                        # ranges the last zero_grad left un-zeroed (the backward overwrites them)
        self.step_count = 0
        self.opt_m = None
        self.opt_v = None
        self.ema = None            # flat fp32 average of the master (ema_update), None until first use
        self.ul_exclude = None     # int64 device ids the unlikelihood term never takes as candidates (set_ul_exclude)
        self.normsq = torch.zeros(1, device=self.dev)
        self.group_normsq = None   # [ngroups + 1] of a grouped step (group_norm_sq); normsq is then its last element
        self.bucket_hook = None   # callable(pack_index) fired as packs of gradients become final
        self._sums, self._defer = [], False     # deferred column sums of the backward (see _defer_sum)
        self._tail_jobs, self._tail_side = [], None      # grouped weight gradients deferred to the backward's tail (_WGRAD_TAIL)
        self._side, self._events = None, {}     # the side stream of the weight-gradient launches and its per-block events
        self._rowmaps = {}

    # ---------------------------------------------------------------- buffers / views
    def set_table(self, table):
        """WenLan token table E[V, emb] (reference: host dict token_id2emb, model.py:215,221-223)."""
        if table is None:
            self.table = None
            return
        t = torch.as_tensor(table)
        if t.shape[1] != self.sh.E:
            raise ValueError("token table width %d != wenlan_emb_size %d" % (t.shape[1], self.sh.E))
        if self.dtype == hip.F32:
            self.table = t.to(self.dev, torch.float32).contiguous()
        else:       # a packed bf16 table goes to the device as it is (54.5 MB, no fp32 detour)
            self.table = t.to(self.dev).to(torch.bfloat16).contiguous()

    def buf(self, name, shape, dtype=None, zero=False):
        """Named workspace.  One allocation per (name, dtype), sized for the largest request seen so far (rounded up
        on a coarse grid) and handed out as a ``[:numel].view(shape)`` slice: the curriculum filter (train.py:178-186)
        changes the row count on almost every step of stages 1 and 2, and a buffer set per exact shape would grow
        without bound (0.3 MB per token at the full configuration).  Every kernel takes its row count and leading
        dimensions explicitly, so a slice of a larger allocation is as good as an exact one."""
        dtype = self.tdt if dtype is None else dtype
        n = 1
        for d in shape:
            n *= int(d)
        key = (name, dtype)
        t = self.ws.get(key)
        if t is None or t.numel() < n:
            cap = _round_capacity(n)
            t = torch.zeros(cap, device=self.dev, dtype=dtype) if zero else torch.empty(cap, device=self.dev, dtype=dtype)
            self.ws[key] = t
            return t[:n].view(shape)
        v = t[:n].view(shape)
        if zero:
            v.zero_()
        return v

    def P(self, key):   # fp32 master view
        return self.layout.view(self.master, key)

    def W(self, key):   # compute-dtype weight view
        return self.layout.view(self.wc, key)

    def G(self, key):   # fp32 gradient view
        return self.layout.view(self.grad, key)

    def Wp(self, pack):
        return self.layout.pack(self.wc, pack)

    def Pp(self, pack):
        return self.layout.pack(self.master, pack)

    def Gp(self, pack):
        return self.layout.pack(self.grad, pack)

    def ensure_grad(self):
        if self.grad is None:
            self.grad = torch.zeros(self.layout.total, device=self.dev, dtype=torch.float32)

    def zero_grad(self, shape_key=None):
        """Zero the flat gradient buffer.  With a shape key (the fused trainer: rows x positions of the step) only what is
        ACCUMULATED into is zeroed once a step of that shape has shown which tensors its backward OVERWRITES (the slab-sum
        block matrices, recorded by _wgrad: 340 of 497 MB at the full configuration) -- one launch over the complement."""
        self.ensure_grad()
        self._ow_rec = None
        self._lazy = None
        if shape_key is not None:
            ent = self._ow_desc.get(shape_key)
            if ent is not None:
                desc, ranges = ent
                hip.zero_ranges(self.grad, desc, desc.shape[0])
                self._lazy = ranges          # these ranges were NOT zeroed: this step's backward must overwrite them
                return
            if len(self._ow_desc) < 64:
                self._ow_rec = (shape_key, [])          # record this step's overwritten ranges
        self.grad.zero_()

    def _finish_overwrite_record(self):
        """After a recorded backward: the complement of the overwritten ranges becomes the zero list of that step shape."""
        if self._ow_rec is None:
            return
        key, ranges = self._ow_rec
        self._ow_rec = None
        ranges = sorted(r for r in ranges if r[0] % 4 == 0 and r[1] % 4 == 0)
        comp, pos = [], 0
        for off, n in ranges:
            if off < pos:
                return                                # overlapping records: keep zeroing everything
            if off > pos:
                comp.append((pos, off - pos))
            pos = off + n
        if pos < self.layout.total:
            comp.append((pos, self.layout.total - pos))
        if not ranges or any(o % 4 or c % 4 for o, c in comp):
            return
        self._ow_desc[key] = (torch.tensor(comp, dtype=torch.int64, device=self.dev), frozenset(ranges))

    def _init_transposed(self):
        """bf16 mode: K-contiguous [out,in] copies of GPT-2's Conv1D [in,out] weights.  With them every
        forward product is the NT layout (both operands K-contiguous in LDS, one ds_read_b128 per
        fragment); the NN layout reads its K-strided weights with two transposed 8-byte LDS reads per
        fragment and measured 5-15 % slower per product (profiles/r01_v4_gemm_per_shape.log)."""
        self.wt = None
        self.wte_t = None
        self.wt_entries = {}
        if self.dtype == hip.F32 and not self.x3:
            return
        pre, desc, off = "decoder.gpt2.transformer.", [], 0
        for l in range(self.sh.L):
            for nm in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"):
                key = "%sh.%d.%s.weight" % (pre, l, nm)
                soff, shape, n = self.layout.entries[key]
                assert soff % 8 == 0 and shape[0] % 8 == 0 and shape[1] % 8 == 0
                desc.append((soff, shape[0], shape[1], off))
                self.wt_entries[key] = (off, (shape[1], shape[0]), n)
                off += n
        if self.x3:
            # x3: the input gradient of a Linear layer, dy [M,out] W[out,in], needs the [in,out] copy as its K-contiguous operand
            key = "decoder.projector_layer2.weight"
            soff, shape, n = self.layout.entries[key]
            if soff % 8 == 0 and shape[0] % 8 == 0 and shape[1] % 8 == 0:
                desc.append((soff, shape[0], shape[1], off))
                self.wt_entries[key] = (off, (shape[1], shape[0]), n)
                off += n
        # (x3: one more leading dimension, the (hi | lo) plane)
        self.wt = torch.zeros(*((2, off) if self.x3 else (off,)), device=self.dev, dtype=torch.bfloat16)
        self.wt_total = off
        self.wt_desc = torch.tensor(desc, dtype=torch.int64, device=self.dev)
        self.wt_max = (max(d[1] for d in desc), max(d[2] for d in desc))
        # ... and a [D, Vpad] copy of the tied embedding matrix: the LM head's dgrad d_h = dlogits @ wte contracts over the
        # vocabulary, wte's ROW index -- through the copy it is a K-contiguous x K-contiguous product like every other
        # forward / dgrad product (eight-phase kernel).  Its own launch: a shared grid would be sized by its 13440 rows.
        woff = self.layout.pack_range["wte"][0]
        self.wte_t = torch.zeros(*((2,) if self.x3 else ()), self.sh.D, self.layout.Vpad, device=self.dev, dtype=torch.bfloat16)
        self.wte_desc = torch.tensor([(woff, self.layout.Vpad, self.sh.D, 0)], dtype=torch.int64, device=self.dev)

    def Wt(self, key):   # [out, in] copy of a Conv1D weight (bf16 mode)
        if self.x3:
            raise RuntimeError("Engine.Wt: an x3 engine's transposed copies are (hi | lo) plane pairs -- use Wtx()")
        off, shape, n = self.wt_entries[key]
        return self.wt[off:off + n].view(shape)

    def _refresh_transposed(self):
        if self.wt is not None and self.x3:
            for pl in (0, 1):
                hip.transpose_batch(self.wc2[pl], self.wt[pl], self.wt_desc, self.wt_desc.shape[0], *self.wt_max)
                hip.transpose_batch(self.wc2[pl], self.wte_t[pl], self.wte_desc, 1, self.layout.Vpad, self.sh.D)
        elif self.wt is not None:
            hip.transpose_batch(self.wc, self.wt, self.wt_desc, self.wt_desc.shape[0], *self.wt_max)
            hip.transpose_batch(self.wc, self.wte_t, self.wte_desc, 1, self.layout.Vpad, self.sh.D)

    def refresh_copies(self):
        """bf16 mode: re-derive the GEMM weight copies from the fp32 masters (an
        external optimizer may have updated them).  654 MB of traffic, ~0.15 ms.
        x3 mode: the (hi | lo) plane pair of the flat buffer and its transposed copies."""
        if self.copies_fresh:
            return
        if self.x3:
            hip.split_planes(self.master, 1, self.layout.total, hip.Planes(self.wc2, 1, self.layout.total))
            self._refresh_transposed()
            self.copies_fresh = True
        elif self.dtype != hip.F32:
            hip.cast_f32_to(self.master, self.wc, self.layout.total)
            self._refresh_transposed()
            self.copies_fresh = True

    def invalidate_copies(self):
        if self.dtype != hip.F32 or self.x3:
            self.copies_fresh = False

    # ---------------------------------------------------------------- split-precision (x3) operands
    def Wx(self, key):
        """Plane pair of a parameter as stored ([out,in] Linear / [in,out] Conv1D)."""
        off, shape, n = self.layout.entries[key]
        return hip.Planes(self.wc2[0, off:off + n], shape[0], shape[1], plane=self.layout.total)

    def Wtx(self, key):
        """Plane pair of the [out,in] copy of a Conv1D weight."""
        off, shape, n = self.wt_entries[key]
        return hip.Planes(self.wt[0, off:off + n], shape[0], shape[1], plane=self.wt_total)

    def Wpx(self, pack, rows, cols):
        off, n = self.layout.pack_range[pack]
        return hip.Planes(self.wc2[0, off:off + n], rows, cols, plane=self.layout.total)

    def pbuf(self, name, rows, cols):
        """Named (hi | lo) plane-pair workspace of an fp32 [rows, cols] activation."""
        t = self.buf(name, (2, rows, cols), torch.bfloat16)
        return hip.Planes(t, rows, cols)

    def _fwd_x3(self, xp, wkey, out, M, bias=None, planes=None, **kw):
        """x3 forward product through the [out,in] plane pair of a Conv1D weight: out / planes = epi(x W + bias)."""
        w = self.Wtx(wkey)
        hip.gemm_x3(xp, w, out, M, w.rows, w.cols, planes=planes, bias=bias, **kw)

    def _dgrad_x3(self, dyp, wkey, dx, M, planes=None, **kw):
        """x3 input gradient of a Conv1D layer: dy [M,out] W[in,out]^T -- the weight as stored is the K-contiguous operand."""
        w = self.Wx(wkey)
        hip.gemm_x3(dyp, w, dx, M, w.rows, w.cols, planes=planes, **kw)

    # ---------------------------------------------------------------- GEMM helpers
    def _gemm_few_rows(self, A, Bm, out, M, N, K, transB, ldb, bias=None, lda=None):
        """Encoder-sized products (M = B or B*S rows, K >= 1024): a handful of output tiles each walking a long K
        serially leaves most CUs idle, so the bf16 mode splits K into fp32 slabs (deterministic) and lets the
        finish kernel add the bias.  Returns False when the plain launch should be used."""
        if K < 1024 or K % 8 or N % 8 or out.dtype != self.tdt:
            return False
        if self.dtype == hip.F32 and (K % 32 or (lda or K) % 4):
            return False
        # (fp32 kernel, round 5: the same K slabs through its MMTG_EPI_SPLIT epilogue -- 128x128 tiles; the encoder's 2048-deep
        #  products on 6-36 tiles were 2.7 ms of the bf16x3 step at 6 TFLOP/s)
        tiles = (N + 31) // 32 if (transB and M <= 256 and self.dtype == hip.BF16) else ((M + 127) // 128) * ((N + 127) // 128)
        splits = min(K // 256, 384 // tiles)
        if tiles > 48 or splits < 2:
            return False
        part = self.buf("few_rows_slabs", (8 * 320 * 2048,), torch.float32)
        if splits * M * N > part.numel():
            return False
        hip.gemm(A, Bm, part, M, N, K, transB=transB, lda=lda, ldb=ldb, ldc=N, epi=hip.EPI_SPLIT, out_f32=True, splits=splits)
        hip.splitk_finish(part, splits, M, N, out, bias=bias)
        return True

    def _fwd(self, x, wkey, out, M, kind, bias=None, lda=None, **kw):
        """out[M,out] = x[M,in] W (+bias).  kind: 'linear' = [out,in], 'conv1d' = [in,out]."""
        w = self.W(wkey)
        if kind == "linear":
            N, K = w.shape
            if not kw and self._gemm_few_rows(x, w, out, M, N, K, True, K, bias=bias, lda=lda):
                return
            hip.gemm(x, w, out, M, N, K, transB=True, lda=lda, ldb=K, bias=bias, **kw)
        elif wkey in self.wt_entries and not self.x3:   # bf16: the [out,in] copy -> NT layout
            # (an x3 engine's `wt` holds (hi | lo) PLANE PAIRS, read by _fwd_x3 only; its plain products -- the decoder's
            #  MMTG_DECODE_X3=0 / n_embd > 1024 fallback -- take the fp32 weight as stored through the exact-fp32 kernel below)
            K, N = w.shape
            hip.gemm(x, self.Wt(wkey), out, M, N, K, transB=True, lda=lda, ldb=K, bias=bias, **kw)
        else:
            K, N = w.shape
            hip.gemm(x, w, out, M, N, K, transB=False, lda=lda, ldb=N, bias=bias, **kw)

    def _dgrad(self, dy, wkey, dx, M, kind, **kw):
        w = self.W(wkey)
        if kind == "linear":
            K, N = w.shape   # dy [M,out=K] @ W[out,in] -> [M,in=N]
            if not kw and self._gemm_few_rows(dy, w, dx, M, N, K, False, N):
                return
            hip.gemm(dy, w, dx, M, N, K, transB=False, ldb=N, **kw)
        else:
            N, K = w.shape   # dy [M,out=K] @ W[in,out]^T -> [M,in=N]
            hip.gemm(dy, w, dx, M, N, K, transB=True, ldb=K, **kw)

    def _wgrad(self, x, dy, wkey, bkey, Mtok, kind, ldx=None, ldy=None, bias_rows=None):
        gw = self.G(wkey)
        if kind == "linear":    # gw[out,in] += dy^T x
            out_f, in_f = gw.shape
            A, B, Mg, Ng, lda, ldb = dy, x, out_f, in_f, ldy or out_f, ldx or in_f
        else:                   # Conv1D: gw[in,out] += x^T dy
            in_f, out_f = gw.shape
            A, B, Mg, Ng, lda, ldb = x, dy, in_f, out_f, ldx or in_f, ldy or out_f
        bf = self.dtype == hip.BF16
        splits = _wgrad_splits(Mg, Ng, Mtok, bf)
        tiles = ((Mg + 127) // 128) * ((Ng + 127) // 128)
        # (the exact-fp32 cross-check mode, round 6: its split weight gradients as slabs too -- any tile count, speed is not its
        #  point -- so that the mode's gradient is bit-reproducible like the others')
        exact = self.dtype == hip.F32 and not self.x3
        use_slab = 1 < splits and Ng % 8 == 0 and ((bf and tiles < 512) or exact)
        if self._lazy is not None and (self.layout.entries[wkey][0], Mg * Ng) in self._lazy and not (use_slab and self.wgrad_overwrite):
            gw.zero_()          # the lazy zero_grad skipped this tensor expecting an overwrite that is not happening now
        if use_slab:
            # K-split slabs with plain stores + an ordered sum instead of fp32 atomics (deterministic)
            # (one workspace, sized for the largest request so far: 113 MB at GPT-2 base, 268 MB at GPT-2 medium)
            part = self.buf("wgrad_slabs", (splits * Mg * Ng,), torch.float32)
            hip.gemm(A, B, part, Mg, Ng, Mtok, transA=True, transB=False, lda=lda, ldb=ldb, ldc=Ng,
                     epi=hip.EPI_SPLIT, out_f32=True, splits=splits)
            # (the fused trainer zeroes the gradients right before its single backward: the sum may then overwrite)
            hip.slab_sum(part, splits, Mg * Ng, gw, Mg * Ng, accumulate=not self.wgrad_overwrite)
            if self.wgrad_overwrite and self._ow_rec is not None:
                self._ow_rec[1].append((self.layout.entries[wkey][0], Mg * Ng))
            splits = 0
        if splits:
            hip.gemm(A, B, gw, Mg, Ng, Mtok, transA=True, transB=False, lda=lda, ldb=ldb, ldc=Ng,
                     epi=hip.EPI_ATOMIC, splits=splits)
        if bkey is not None:
            hip.colsum(dy, Mtok if bias_rows is None else bias_rows, out_f, self.G(bkey), ldx=ldy or out_f)

    # ---------------------------------------------------------------- forward
    def _cast_in(self, t, name):
        """Batch embeddings arrive f64/f32 (model.py:371-373 calls .float()); store in compute dtype."""
        t = t.to(self.dev, torch.float32).contiguous()
        if self.dtype == hip.F32:
            return t
        out = self.buf(name, t.shape)
        hip.cast_f32_to(t, out, t.numel())
        return out

    def _rnn_fwd(self, ch, x, B, training, seed, site):
        """One encoder channel (model.py:39-59, 78-79): `num_layers` stacked GRU / LSTM / ReLU-RNN layers over the S steps, h0 = 0,
        rows b*S+t.  Per layer: W_ih x + b_ih for all steps in ONE product, then per step the recurrent product W_hh h_{t-1} + b_hh
        and the cell kernel; between layers nn.RNNBase's dropout (training only; counter-hash mask, regenerated in the backward).
        Returns the per-layer activation records the backward needs."""
        sh = self.sh
        S, H = sh.S, sh.H
        kind, NL = sh.rnn[ch]
        G = hip.RNN_GATES[kind]
        r = f"encoder.rnns_{ch}."
        gh = self.buf("gh%d" % G, (B, G * H))
        layers, inp = [], x
        for l in range(NL):
            sfx = "_l%d" % l
            tag = ch if l == 0 else "%s%d" % (ch, l)
            gi = self.buf("gi_" + tag, (B * S, G * H))
            self._fwd(inp, r + "weight_ih" + sfx, gi, B * S, "linear", bias=self.P(r + "bias_ih" + sfx))
            h_all = self.buf("h_" + tag, (B * S, H))
            rec = {"inp": inp, "gi": gi, "h": h_all, "drop": None}
            if kind == "GRU":
                save = rec["save"] = self.buf("gru_save_" + tag, (S, 4, B, H), torch.float32)
                for t in range(S):
                    if t == 0:      # h_prev = 0: the recurrent product is b_hh itself (one row, stride 0), no launch
                        hip.gru_cell_fwd(gi[t:], self.W(r + "bias_hh" + sfx), None, h_all[t:], save[t], B, H,
                                         ld_gi=S * 3 * H, ld_hp=S * H, ld_h=S * H, ld_gh=0)
                        continue
                    self._fwd(h_all[t - 1:], r + "weight_hh" + sfx, gh, B, "linear", bias=self.P(r + "bias_hh" + sfx), lda=S * H)
                    hip.gru_cell_fwd(gi[t:], gh, h_all[t - 1:], h_all[t:], save[t], B, H,
                                     ld_gi=S * 3 * H, ld_hp=S * H, ld_h=S * H)
            else:
                lstm = kind == "LSTM"
                code = hip.RNN_LSTM if lstm else hip.RNN_RELU
                save = rec["save"] = self.buf("lstm_save_" + tag, (S, 5, B, H), torch.float32) if lstm else None
                c_all = rec["c"] = self.buf("lstm_c_" + tag, (S, B, H), torch.float32) if lstm else None
                for t in range(S):
                    if t == 0:
                        g_t, ld_gh = self.W(r + "bias_hh" + sfx), 0
                    else:
                        self._fwd(h_all[t - 1:], r + "weight_hh" + sfx, gh, B, "linear", bias=self.P(r + "bias_hh" + sfx), lda=S * H)
                        g_t, ld_gh = gh, None
                    hip.rnn_cell_fwd(code, gi[t:], g_t, c_all[t - 1] if lstm and t else None, h_all[t:], c_all[t] if lstm else None,
                                     save[t] if lstm else None, B, H, ld_gi=S * G * H, ld_h=S * H, ld_gh=ld_gh)
            layers.append(rec)
            inp = h_all
            if l + 1 < NL and training and sh.rnn_pdrop > 0.0:
                rec["drop"] = mix_seed(seed, 0x1000 + 64 * site + l)
                inp = self.buf("hd_" + tag, (B * S, H))
                hip.dropout_apply(h_all, inp, B * S * H, sh.rnn_pdrop, rec["drop"])
        return layers

    def forward(self, batch, train_flag=True, training=False, per_row_infer=True, need_logits=True, logits_f32=True,
                encode_only=False, exp_drop=None):
        """MMTG.forward (model.py:356-400).  Returns dict(logits_pad [M,Vpad] f32, B, T, ...);
        lm_loss / kl are device scalars in self.scalars after loss().  need_logits=False stops after the last block's c_attn (no ln_f, no
        LM head: the decoder's prompt prefill reads the blocks' K / V rows only); encode_only=True stops after the fuser.
        exp_drop: None or (p_both, p_img, p_txt), the probabilities with which a sample's images and texts, its images alone or its
        texts alone are replaced by zeros (mmtg_experience_drop: what generate.without_experience feeds the decoders); it acts
        whenever it is given and not all zero, whatever `training` says, and leaves the int32 codes in act["exp_drop"]."""
        sh = self.sh
        if self.table is None:
            raise RuntimeError("no WenLan token table set (vocab/token_id2emb_dict.pkl or set_token_table())")
        self.refresh_copies()
        self.training = training
        pe, pa, pr = sh.pdrop if training else (0.0, 0.0, 0.0)
        self.drop_seed = (self.drop_seed * 1664525 + 1013904223) & 0xFFFFFFFF
        seed = self.drop_seed
        S, E, H, D, P = sh.S, sh.E, sh.H, sh.D, sh.P
        img = batch["img_embs"]
        B = img.shape[0]
        if img.shape[1] != S:
            raise ValueError("batch has %d experience steps, model_cfgs['seq_len'] = %d" % (img.shape[1], S))
        if encode_only:          # decode: only the experience vectors c[B,S,E] are needed
            targets = topic_ids = None
            L = T = M = 0
        else:
            targets = batch["targets"].to(self.dev, torch.long).contiguous()
            topic_ids = batch["topic_ids"].to(self.dev, torch.long).contiguous()
            L = targets.shape[1]
            T = P + L
            M = B * T
            if T > sh.NP:
                raise ValueError("sequence length %d exceeds n_positions %d" % (T, sh.NP))
        a = {"B": B, "L": L, "T": T, "M": M, "seed": seed, "pdrop": (pe, pa, pr), "train_flag": train_flag,
             "targets": targets, "topic_ids": topic_ids}

        # ---------------- encoder: topic_fc + 2 GRUs (model.py:63-81) + ln_layer1..3 (:380-382)
        xt = self._cast_in(batch["topic_emb"], "xt")
        if exp_drop is not None and any(p > 0.0 for p in exp_drop):
            # one launch casts both channels and zeroes the dropped samples' rows; always into the engine's own buffers (the f32
            # modes pass the caller's tensors on otherwise).  The backward needs nothing: the layer records keep these as `inp`.
            src_i = img.to(self.dev, torch.float32).contiguous()
            src_r = batch["r_embs"].to(self.dev, torch.float32).contiguous()
            xi, xr = self.buf("xi", (B * S, E)), self.buf("xr", (B * S, E))
            a["exp_drop"] = self.buf("exp_drop_code", (B,), torch.int32)
            hip.experience_drop(src_i, src_r, xi, xr, a["exp_drop"], B, S * E, mix_seed(seed, EXP_DROP_SITE), hip.drop_thresholds(exp_drop))
        else:
            xi = self._cast_in(img, "xi").view(B * S, E)
            xr = self._cast_in(batch["r_embs"], "xr").view(B * S, E)
        t_raw = self.buf("t_raw", (B, H))
        self._fwd(xt, "encoder.topic_fc.weight", t_raw, B, "linear", bias=self.P("encoder.topic_fc.bias"))
        t_ln = self.buf("t_ln", (B, H))
        st = {}
        st["ln1"] = (self.buf("ln1_mu", (B,), torch.float32), self.buf("ln1_rs", (B,), torch.float32))
        hip.layernorm_fwd(t_raw, t_ln, self.P("ln_layer1.weight"), self.P("ln_layer1.bias"), *st["ln1"], B, H)
        enc = {}
        for ch, x, lnk, site in (("image", xi, "ln_layer2", 0), ("text", xr, "ln_layer3", 1)):
            layers = self._rnn_fwd(ch, x, B, training, seed, site)
            h_all = layers[-1]["h"]
            h_ln = self.buf("hln_" + ch, (B * S, H))
            st[lnk] = (self.buf(lnk + "_mu", (B * S,), torch.float32), self.buf(lnk + "_rs", (B * S,), torch.float32))
            hip.layernorm_fwd(h_all, h_ln, self.P(lnk + ".weight"), self.P(lnk + ".bias"), *st[lnk], B * S, H)
            enc[ch] = (layers, h_ln)

        # ---------------- alpha attention (model.py:133-161) on batch-first rows b*S+i
        kl = self.buf("kl", (1,), torch.float32, zero=True)
        alpha = {}
        for mod, ch in (("img", "image"), ("text", "text")):
            h_ln = enc[ch][1]
            qkv = self.buf("aqkv_" + mod, (B * S, 3 * H))
            hip.gemm(h_ln, self.Wp(mod + "_qkv_w"), qkv, B * S, 3 * H, H, transB=True, ldb=H, bias=self.Pp(mod + "_qkv_b"))
            ctx = self.buf("actx_" + mod, (B * S, H))
            probs = self.buf("aprobs_" + mod, (B, sh.heads, S, S), torch.float32)
            hip.alpha_attn_fwd(qkv, self.prior, ctx, probs, kl, B, S, H, sh.heads)
            alpha[mod] = (qkv, ctx, probs)

        # ---------------- beta fuser (model.py:181-202) -> c [B,S,E]
        o = self.buf("beta_o", (B * S, H))
        ba = self.buf("beta_a", (B, S, 3), torch.float32)
        hip.beta_fuse_fwd(t_ln, alpha["img"][1], alpha["text"][1], self.Pp("att_w"), self.Pp("att_b"), o, ba, B, S, H)
        c = self.buf("c", (B * S, E))
        self._fwd(o, "mm_atten_layer.out_linear.weight", c, B * S, "linear", bias=self.P("mm_atten_layer.out_linear.bias"))

        if encode_only:
            a.update(c=c, kl=kl)
            self.act = a
            return a
        # ---------------- decoder front end (model.py:251-281) + GPT-2 input embedding
        if train_flag:
            type_ids = torch.cat([batch["tpw_type_ids"].to(self.dev).long(), batch["type_ids"].to(self.dev).long()], 1)
            keep = torch.cat([batch["tpw_attention_mask"].to(self.dev), batch["attention_mask"].to(self.dev)], 1)
        else:
            type_ids, keep = self._infer_types_mask(batch, targets, per_row_infer)
        type_ids = type_ids.contiguous().view(-1)
        keep = (keep != 0).to(torch.int32).contiguous()
        h1 = self.buf("h1", (M, H))
        px3 = self.x3 and E % 128 == 0 and H % 128 == 0 and D % 8 == 0 and "decoder.projector_layer2.weight" in self.wt_entries
        a["px3"] = px3
        gather = self.dtype == hip.BF16 and M > 256
        if gather:
            # Fused conditioning (model.py:254-281): X[m] = E[id_m] + c[b, seg_m] is never materialised.  By linearity
            # X W1^T = E[id] W1^T + (c W1^T)[b, seg]: the projector product gathers its A rows straight from the WenLan table
            # (the row index is the LDS-DMA lane's source offset) and its epilogue adds row b*S + seg of the small product
            # c W1^T (row B*S = zeros for the prompt and the positions past the last segment) before the tanh.
            ids32 = torch.cat([topic_ids, targets], 1).to(torch.int32).contiguous().view(-1)
            rowmap = self._rowmaps.get((B, T))
            if rowmap is None:          # depends on the shapes only: built once per (B, T)
                lp = torch.arange(T, device=self.dev) - P
                seg = torch.div(lp, sh.two_sents, rounding_mode="floor")
                seg = torch.where((lp >= 0) & (seg < S), seg, torch.full_like(seg, -1))
                rowmap = torch.where(seg >= 0, torch.arange(B, device=self.dev)[:, None] * S + seg[None, :],
                                     torch.full((B, T), B * S, device=self.dev)).to(torch.int32).contiguous().view(-1)
                if len(self._rowmaps) > 256:
                    self._rowmaps.clear()
                self._rowmaps[(B, T)] = rowmap
            cW = self.buf("c_w1", (B * S + 1, H))
            self._fwd(c, "decoder.projector_layer1.weight", cW[:B * S], B * S, "linear")
            cW[B * S:].zero_()
            hip.gemm_gather(0, self.table, self.W("decoder.projector_layer1.weight"), h1, M, H, E, ids32, self.table.shape[0],
                            lda=E, ldb=E, bias=self.P("decoder.projector_layer1.bias"), epi=hip.EPI_TANH_ADD, aux=cW, ldaux=H,
                            aux_rows=rowmap)
            x = None
        else:
            ids32 = None
            x = self.buf("x_cond", (M, E))
            hip.embed_condition(self.table, topic_ids, targets, c, x, B, P, L, S, E, sh.two_sents, self.table.shape[0])
            if px3:
                # split-precision projector (model.py:279-281): X and tanh(X W1^T + b1) also as plane pairs (the products' operands)
                xp = hip.split_planes(x, M, E, self.pbuf("x_cond_p", M, E))
                h1p = self.pbuf("h1_p", M, H)
                hip.gemm_x3(xp, self.Wx("decoder.projector_layer1.weight"), h1, M, H, E, planes=h1p,
                            bias=self.P("decoder.projector_layer1.bias"), epi=hip.EPI_TANH)
                a.update(xp=xp, h1p=h1p)
            else:
                self._fwd(x, "decoder.projector_layer1.weight", h1, M, "linear", bias=self.P("decoder.projector_layer1.bias"),
                          epi=hip.EPI_TANH)
        hcur = self.buf("resid_0", (M, D))
        if px3:
            hip.gemm_x3(a["h1p"], self.Wx("decoder.projector_layer2.weight"), hcur, M, D, H, bias=self.P("decoder.projector_layer2.bias"))
        else:
            self._fwd(h1, "decoder.projector_layer2.weight", hcur, M, "linear", bias=self.P("decoder.projector_layer2.bias"))
        pre = "decoder.gpt2.transformer."
        hip.embed_add(hcur, self.W(pre + "wpe.weight"), self.W(pre + "wte.weight"), type_ids, hcur, M, T, D,
                      drop_p=pe, drop_seed=seed)

        # ---------------- GPT-2 blocks
        layers = []
        x3 = self.x3 and D % 128 == 0
        a["x3"] = x3
        for l in range(sh.L):
            p = f"{pre}h.{l}."
            s = (mix_seed(seed, 3 * l + 1), mix_seed(seed, 3 * l + 2), mix_seed(seed, 3 * l + 3))   # attn, resid 1, resid 2
            mu1 = self.buf(f"l{l}_mu1", (M,), torch.float32)
            rs1 = self.buf(f"l{l}_rs1", (M,), torch.float32)
            mu2 = self.buf(f"l{l}_mu2", (M,), torch.float32)
            rs2 = self.buf(f"l{l}_rs2", (M,), torch.float32)
            if x3:
                # split-precision block: the LayerNorms, c_attn and the GELU write (hi | lo) plane pairs -- only products and the
                # split-precision attention read them -- the attention context is needed in fp32 by its backward's delta AND as
                # planes by c_proj
                a1 = self.pbuf(f"l{l}_a", M, D)
                hyb = self.hybrid
                # (hybrid: the LayerNorm kernels also store their input rows as bf16 -- what the bf16 LayerNorm backward reads)
                xb1 = self.buf(f"l{l}_xin_b", (M, D), torch.bfloat16) if hyb else None
                xb2 = self.buf(f"l{l}_xmid_b", (M, D), torch.bfloat16) if hyb else None
                hip.layernorm_fwd_x3(hcur, a1, self.P(p + "ln_1.weight"), self.P(p + "ln_1.bias"), mu1, rs1, M, D, sh.eps, xb=xb1)
                qkv = self.pbuf(f"l{l}_qkvp", M, 3 * D)
                self._fwd_x3(a1, p + "attn.c_attn.weight", None, M, bias=self.P(p + "attn.c_attn.bias"), planes=qkv, ldc=3 * D)
                if not need_logits and l == sh.L - 1:      # (the prefill wants K / V only: nothing of the last block beyond c_attn)
                    layers.append((hcur, mu1, rs1, a1, qkv))
                    break
                ctx = self.buf(f"l{l}_ctx", (M, D))
                lse = self.buf(f"l{l}_lse", (B, sh.nH, T), torch.float32)
                ctxp = self.pbuf(f"l{l}_ctxp", M, D)
                hip.attn_fwd_x3(qkv, keep, ctx, ctxp, lse, B, T, sh.nH, D // sh.nH, drop_p=pa, drop_seed=s[0])
                xmid = self.buf(f"l{l}_xmid", (M, D))
                self._fwd_x3(ctxp, p + "attn.c_proj.weight", xmid, M, bias=self.P(p + "attn.c_proj.bias"),
                             epi=hip.EPI_RESID, aux=hcur, ldaux=D, drop_p=pr, drop_seed=s[1])
                m2 = self.pbuf(f"l{l}_m", M, D)
                hip.layernorm_fwd_x3(xmid, m2, self.P(p + "ln_2.weight"), self.P(p + "ln_2.bias"), mu2, rs2, M, D, sh.eps, xb=xb2)
                # (hybrid: the saved pre-activation as bf16 rows, the bf16 dGELU epilogue's operand -- half the bytes, too)
                u = self.buf(f"l{l}_u_b" if hyb else f"l{l}_u", (M, 4 * D), torch.bfloat16 if hyb else None)
                gact = self.pbuf(f"l{l}_g", M, 4 * D)
                self._fwd_x3(m2, p + "mlp.c_fc.weight", None, M, bias=self.P(p + "mlp.c_fc.bias"), planes=gact, ldc=4 * D,
                             epi=hip.EPI_GELU, aux2=u, flags=hip.GEMM_AUX2_BF16 if hyb else 0)
                xout = self.buf(f"resid_{l + 1}", (M, D))
                self._fwd_x3(gact, p + "mlp.c_proj.weight", xout, M, bias=self.P(p + "mlp.c_proj.bias"),
                             epi=hip.EPI_RESID, aux=xmid, ldaux=D, drop_p=pr, drop_seed=s[2])
                layers.append((hcur, mu1, rs1, a1, qkv, ctx, lse, xmid, mu2, rs2, m2, u, gact, s, ctxp))
                if hyb:
                    a.setdefault("hyb_rows", []).append((xb1, xb2))
                hcur = xout
                continue
            a1 = self.buf(f"l{l}_a", (M, D))
            hip.layernorm_fwd(hcur, a1, self.P(p + "ln_1.weight"), self.P(p + "ln_1.bias"), mu1, rs1, M, D, sh.eps)
            qkv = self.buf(f"l{l}_qkv", (M, 3 * D))
            self._fwd(a1, p + "attn.c_attn.weight", qkv, M, "conv1d", bias=self.P(p + "attn.c_attn.bias"))
            if not need_logits and l == sh.L - 1:          # (the prefill wants K / V only: nothing of the last block beyond c_attn)
                layers.append((hcur, mu1, rs1, a1, qkv))
                break
            ctx = self.buf(f"l{l}_ctx", (M, D))
            lse = self.buf(f"l{l}_lse", (B, sh.nH, T), torch.float32)
            hip.attn_fwd(qkv, keep, ctx, lse, B, T, sh.nH, D // sh.nH, drop_p=pa, drop_seed=s[0])
            xmid = self.buf(f"l{l}_xmid", (M, D))
            self._fwd(ctx, p + "attn.c_proj.weight", xmid, M, "conv1d", bias=self.P(p + "attn.c_proj.bias"),
                      epi=hip.EPI_RESID, aux=hcur, ldaux=D, drop_p=pr, drop_seed=s[1])
            m2 = self.buf(f"l{l}_m", (M, D))
            hip.layernorm_fwd(xmid, m2, self.P(p + "ln_2.weight"), self.P(p + "ln_2.bias"), mu2, rs2, M, D, sh.eps)
            u = self.buf(f"l{l}_u", (M, 4 * D))
            gact = self.buf(f"l{l}_g", (M, 4 * D))
            # (u: the pre-activation, which the dGELU epilogue of the backward reads)
            self._fwd(m2, p + "mlp.c_fc.weight", gact, M, "conv1d", bias=self.P(p + "mlp.c_fc.bias"),
                      epi=hip.EPI_GELU, aux2=u)
            xout = self.buf(f"resid_{l + 1}", (M, D))
            self._fwd(gact, p + "mlp.c_proj.weight", xout, M, "conv1d", bias=self.P(p + "mlp.c_proj.bias"),
                      epi=hip.EPI_RESID, aux=xmid, ldaux=D, drop_p=pr, drop_seed=s[2])
            layers.append((hcur, mu1, rs1, a1, qkv, ctx, lse, xmid, mu2, rs2, m2, u, gact, s, None))
            hcur = xout
        if not need_logits:      # the decoder's prompt prefill: only the blocks' K / V rows (layers[l][4]) are wanted
            a.update(c=c, kl=kl, type_ids=type_ids, keep=keep, layers=layers, x_last=hcur, logits=None)
            self.act = a
            return a
        muf = self.buf("lnf_mu", (M,), torch.float32)
        rsf = self.buf("lnf_rs", (M,), torch.float32)
        Vp = self.layout.Vpad
        # fp32 logits for the reference-shaped surface (MMTG.forward returns them); the fused trainer of the
        # bf16 mode keeps them in bf16 like every other activation (logits_f32=False)
        l32 = logits_f32 or self.dtype == hip.F32
        logits = self.buf("logits" if l32 else "logits_c", (M, Vp), torch.float32 if l32 else self.tdt)
        if x3:
            hf = self.pbuf("hf", M, D)
            if self.hybrid:
                a["x_last_b"] = self.buf("x_last_b", (M, D), torch.bfloat16)
            hip.layernorm_fwd_x3(hcur, hf, self.P(pre + "ln_f.weight"), self.P(pre + "ln_f.bias"), muf, rsf, M, D, sh.eps, xb=a.get("x_last_b"))
            hip.gemm_x3(hf, self.Wpx("wte", Vp, D), logits, M, Vp, D)
        else:
            hf = self.buf("hf", (M, D))
            hip.layernorm_fwd(hcur, hf, self.P(pre + "ln_f.weight"), self.P(pre + "ln_f.bias"), muf, rsf, M, D, sh.eps)
            hip.gemm(hf, self.Wp("wte"), logits, M, Vp, D, transB=True, ldb=D, out_f32=l32)
        a.update(xt=xt, t_raw=t_raw, t_ln=t_ln, st=st, enc=enc, alpha=alpha, kl=kl, o=o, ba=ba, c=c, x=x, ids32=ids32, h1=h1,
                 type_ids=type_ids, keep=keep, layers=layers, x_last=hcur, muf=muf, rsf=rsf, hf=hf, logits=logits)
        self.act = a
        return a

    def _infer_types_mask(self, batch, targets, per_row):
        """Inference branch of GPT2_Decoder.forward (model.py:290-312), vectorised: lyric
        position i has type 0 if (i+1) % sent in {0,1} or the token is PAD, else
        [1..max_sent_num-1, 1][i // sent]; mask 0 on PAD.  The reference decides from row 0
        only (batch 1); per_row=True applies the rule to every row (batched decode)."""
        sh = self.sh
        sent = sh.msl + 2
        n = targets.shape[1]
        Bn = targets.shape[0]
        src = targets if per_row else targets[:1].expand(Bn, n)
        tlist = list(range(1, sh.max_seq_length // sent + 1)) + [1]
        idx = torch.arange(n, device=self.dev)
        slot = torch.tensor([tlist[min(i // sent, len(tlist) - 1)] for i in range(n)], device=self.dev, dtype=torch.long)
        edge = ((idx + 1) % sent == 0) | ((idx + 1) % sent == 1)
        is_pad = src == 0
        types = torch.where(edge[None, :] | is_pad, torch.zeros_like(src), slot[None, :].expand(Bn, n))
        mask = (~is_pad).long()
        return (torch.cat([batch["tpw_type_ids"].to(self.dev).long(), types], 1),
                torch.cat([batch["tpw_attention_mask"].to(self.dev).long(), mask], 1))

    # ---------------------------------------------------------------- loss
    def loss(self, ratings=None, stage=3, batch_den=None, label_zero=False):
        """MyLoss (loss.py:45-74) + GPT-2's internal LM loss on the forward's logits.
        scalars[0] = MyLoss, scalars[1] = LM loss; also fills coef for loss_backward()."""
        a, sh = self.act, self.sh
        B, L, M = a["B"], a["L"], a["M"]
        nll = self.buf("nll", (M,), torch.float32)
        lse = self.buf("lse_rows", (M,), torch.float32)
        ce = self.buf("sample_ce", (B,), torch.float32)
        coef = self.buf("coef", (B,), torch.float32)
        sc = self.buf("loss_scalars", (2,), torch.float32)
        r = None if ratings is None else ratings.to(self.dev, torch.long).contiguous()
        hip.loss_fwd(a["logits"], self.layout.Vpad, sh.V, a["topic_ids"], a["targets"], r, stage, label_zero,
                     B, sh.P, L, float(B if batch_den is None else batch_den), nll, lse, ce, coef, sc)
        a.update(nll=nll, lse_rows=lse, sample_ce=ce, coef=coef, scalars=sc)
        return sc

    def loss_backward(self, gscale=1.0, lm_coef=0.0):
        """d(gscale * MyLoss + lm_scale * LM loss)/d logits into the engine's dlogits buffer."""
        a, sh = self.act, self.sh
        if a.get("x3") and self.hybrid:
            # hybrid: fp32 logits in, the gradient as bf16 rows (the bf16 backward's LM-head operand)
            dl = self.buf("dlogits_b", (a["M"], self.layout.Vpad), torch.bfloat16)
            hip.loss_bwd(a["logits"], self.layout.Vpad, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"],
                         gscale, a["B"], sh.P, a["L"], dl, self.layout.Vpad, self.layout.Vpad, lm_coef=lm_coef)
            return dl
        if a.get("x3"):
            # x3: the gradient goes straight into the plane pair the LM head's split-precision products read
            dlp = self.pbuf("dlogits_p", a["M"], self.layout.Vpad)
            hip.loss_bwd_x3(a["logits"], self.layout.Vpad, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"],
                            gscale, a["B"], sh.P, a["L"], dlp, self.layout.Vpad, lm_coef=lm_coef)
            return dlp
        # compute-dtype logits are overwritten in place by their gradient
        dl = a["logits"] if a["logits"].dtype == self.tdt and self.dtype != hip.F32 else self.buf("dlogits", (a["M"], self.layout.Vpad))
        hip.loss_bwd(a["logits"], self.layout.Vpad, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"],
                     gscale, a["B"], sh.P, a["L"], dl, self.layout.Vpad, self.layout.Vpad, lm_coef=lm_coef)
        return dl

    # ---- token-level unlikelihood on repeated lyric tokens (the rule: include/mmtg_hip.h; MMTGTrainer(ul_weight=...))
    def set_ul_exclude(self, ids):
        """The ids that are never candidates (at most 32), uploaded once."""
        ids = [int(i) for i in ids]
        self.ul_exclude = torch.tensor(ids, device=self.dev, dtype=torch.long) if ids else None

    def ul_loss(self, batch_den=None):
        """The term on the forward's logits, after loss() (it reads the row lse): the device scalar ul [1]; also fills the row sums
        S for loss_backward_ul()."""
        a, sh = self.act, self.sh
        B, L, M = a["B"], a["L"], a["M"]
        row = self.buf("ul_row", (M,), torch.float32)
        S = self.buf("ul_S", (M,), torch.float32)
        smp = self.buf("ul_sample", (B,), torch.float32)
        ul = self.buf("ul_scalar", (1,), torch.float32)
        hip.loss_ul_fwd(a["logits"], self.layout.Vpad, sh.V, a["targets"], a["lse_rows"], self.ul_exclude,
                        B, sh.P, L, float(B if batch_den is None else batch_den), row, S, smp, ul)
        a.update(ul_row=row, ul_S=S, ul_sample=smp, ul=ul)
        return ul

    def loss_backward_ul(self, gscale=1.0, lm_coef=0.0, ul_coef=0.0):
        """loss_backward() with ul_coef * d(sum of the row terms)/d logits added, ul_coef = ul_weight * gscale / (ntok * batch_den);
        the same buffers and storage forms."""
        a, sh = self.act, self.sh
        Vp, ex = self.layout.Vpad, self.ul_exclude
        args = (a["logits"], Vp, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"], gscale, a["ul_S"], ul_coef, ex,
                a["B"], sh.P, a["L"])
        if a.get("x3") and self.hybrid:
            dl = self.buf("dlogits_b", (a["M"], Vp), torch.bfloat16)
            hip.loss_bwd_ul(*args, dl, Vp, Vp, lm_coef=lm_coef)
            return dl
        if a.get("x3"):
            dlp = self.pbuf("dlogits_p", a["M"], Vp)
            hip.loss_bwd_ul_x3(*args, dlp, Vp, lm_coef=lm_coef)
            return dlp
        dl = a["logits"] if a["logits"].dtype == self.tdt and self.dtype != hip.F32 else self.buf("dlogits", (a["M"], Vp))
        hip.loss_bwd_ul(*args, dl, Vp, Vp, lm_coef=lm_coef)
        return dl

    # ---- contrastive token loss on the last-layer states (the rule: include/mmtg_hip.h; MMTGTrainer(cl_weight=...))
    def cl_loss(self, margin, batch_den=None):
        """The term on the forward's ln_f output and keep mask: the device scalar cl [1]; also fills the row reciprocals that
        backward(cl_coef=...) reads.  The bf16 and f32 modes pass hf as it is; the x3 modes join its (hi | lo) planes into an fp32
        [M, D] buffer first (hi + lo is exact in fp32: two casts and one axpy_f32) and run the f32 form."""
        a, sh = self.act, self.sh
        B, L, M, D = a["B"], a["L"], a["M"], sh.D
        hf = a["hf"]
        if isinstance(hf, hip.Planes):
            h32 = self.buf("cl_hf32", (M, D), torch.float32)
            lo = self.buf("cl_lo32", (M, D), torch.float32)
            hip.cast_to_f32(hf.t[0], h32, M * D)
            hip.cast_to_f32(hf.t[1], lo, M * D)
            hip.axpy_f32(h32, lo, 1.0, M * D)
            hf = h32
        rinv = self.buf("cl_rinv", (M,), torch.float32)
        row = self.buf("cl_row", (M,), torch.float32)
        smp = self.buf("cl_sample", (B,), torch.float32)
        cl = self.buf("cl_scalar", (1,), torch.float32)
        hip.cl_fwd(hf, D, a["keep"], sh.P + L, margin, B, sh.P, L, D, float(B if batch_den is None else batch_den), rinv, row, smp, cl)
        a.update(cl_hf=hf, cl_rinv=rinv, cl_row=row, cl_sample=smp, cl=cl, cl_margin=float(margin))
        return cl

    def _cl_record(self, a, cl_coef, cl_margin):
        """What _backward_decoder hands to hip.cl_bwd: (hf as cl_loss read it, rinv, margin, coef)."""
        if "cl_rinv" not in a:
            raise RuntimeError("backward(cl_coef > 0) needs cl_loss() on this forward")
        return (a["cl_hf"], a["cl_rinv"], a["cl_margin"] if cl_margin is None else float(cl_margin), float(cl_coef))

    # ---- the guided validation loss (the rule: include/mmtg_hip.h; MMTGTrainer.evaluate_guided)
    def guided_loss(self, scales, uncond_logits, uncond_lse, batch_den=None):
        """After forward() and loss() on the conditional batch: the cross-entropy of the lyric under softmax(lu + s (lc - lu)) for the
        K <= 8 scales, with the unconditional branch's logits [M, Vpad] (the storage type of this forward's, a buffer of the caller's
        own: the engine's were overwritten by this forward) and their row lse [M].  Returns the device tensor ce [K]; nll [K, M] and
        sample_ce [K, B] are recorded in act."""
        a, sh = self.act, self.sh
        B, L, M, K = a["B"], a["L"], a["M"], len(scales)
        if "lse_rows" not in a:
            raise RuntimeError("guided_loss() needs loss() on this forward (it reads the row lse)")
        lg = a["logits"]
        if uncond_logits.dtype != lg.dtype or uncond_logits.numel() != lg.numel() or uncond_lse.numel() != M:
            raise ValueError("guided_loss: the unconditional logits and lse must have the conditional forward's type and shape")
        nll = self.buf("guided_nll", (K, M), torch.float32)
        smp = self.buf("guided_sample_ce", (K, B), torch.float32)
        ce = self.buf("guided_ce", (K,), torch.float32)
        hip.guided_loss(lg, uncond_logits, self.layout.Vpad, sh.V, a["lse_rows"], uncond_lse, a["topic_ids"], a["targets"], scales,
                        B, sh.P, L, float(B if batch_den is None else batch_den), nll, smp, ce)
        a.update(guided_nll=nll, guided_sample_ce=smp, guided_ce=ce)
        return ce

    def guided_loss_multi(self, scale_tuples, neg_logits, neg_lses, batch_den=None):
        """After forward() and loss() on the conditional batch: the cross-entropy of the lyric under lc + sum_k (s_k - 1) (lc - l_k),
        what ModalityGuidedDecoder selects from, for the G <= 8 tuples of len(neg_logits) scales each, with the 1 .. 3 running
        negatives' logits [M, Vpad] (the storage type of this forward's, buffers of the caller's own) and their row lse [M] in branch
        order.  Returns the device tensor ce [G]; nll [G, M] and sample_ce [G, B] are recorded in act."""
        a, sh = self.act, self.sh
        B, L, M, G = a["B"], a["L"], a["M"], len(scale_tuples)
        if "lse_rows" not in a:
            raise RuntimeError("guided_loss_multi() needs loss() on this forward (it reads the row lse)")
        lg = a["logits"]
        if len(neg_logits) != len(neg_lses) or any(x.dtype != lg.dtype or x.numel() != lg.numel() for x in neg_logits) or any(
                v.numel() != M for v in neg_lses):
            raise ValueError("guided_loss_multi: the negatives' logits and lse must have the conditional forward's type and shape")
        nll = self.buf("guided_nll", (G, M), torch.float32)
        smp = self.buf("guided_sample_ce", (G, B), torch.float32)
        ce = self.buf("guided_ce", (G,), torch.float32)
        hip.guided_loss_multi([lg] + list(neg_logits), [a["lse_rows"]] + list(neg_lses), self.layout.Vpad, sh.V, a["targets"],
                              scale_tuples, B, sh.P, L, float(B if batch_den is None else batch_den), nll, smp, ce)
        a.update(guided_nll=nll, guided_sample_ce=smp, guided_ce=ce)
        return ce

    # ---- distillation of a teacher's (guided) distribution (the rule: include/mmtg_hip.h; MMTGTrainer(distill_weight=...))
    def distill_loss(self, teacher_logits, teacher_lse, uncond_logits=None, uncond_lse=None, scale=1.0, batch_den=None):
        """After forward() and loss(): KL(q || p) of this forward's logits against q = softmax(lu + scale (lc - lu)) of a teacher's
        conditional logits [M, ld] (fp32 or bf16, ld >= V; a teacher engine's own buffer or a copy) with their row lse [M], and the
        negative's logits and lse (buffers of the caller's own, both None: q = softmax(lc)).  Returns the device scalar kd [1];
        kd_row, kd_lg, kd_sample are recorded in act with the teacher's tensors, which loss_backward_kd() reads again."""
        a, sh = self.act, self.sh
        B, L, M = a["B"], a["L"], a["M"]
        if "lse_rows" not in a:
            raise RuntimeError("distill_loss() needs loss() on this forward (it reads the row lse)")
        if teacher_logits.dim() != 2 or teacher_logits.shape[0] != M or teacher_logits.shape[1] < sh.V or teacher_lse.numel() != M:
            raise ValueError("distill_loss: the teacher's logits must be [M = %d, >= V = %d] with M row lse" % (M, sh.V))
        if (uncond_logits is None) != (uncond_lse is None):
            raise ValueError("distill_loss: uncond_logits and uncond_lse are given together or not at all")
        if uncond_logits is not None and (uncond_logits.dtype != teacher_logits.dtype or uncond_logits.shape != teacher_logits.shape
                                          or uncond_lse.numel() != M):
            raise ValueError("distill_loss: the negative's logits and lse must have the teacher's type and shape")
        row = self.buf("kd_row", (M,), torch.float32)
        lg = self.buf("kd_lg", (M,), torch.float32)
        smp = self.buf("kd_sample", (B,), torch.float32)
        kd = self.buf("kd_scalar", (1,), torch.float32)
        ldt = teacher_logits.stride(0)
        hip.distill_fwd(a["logits"], self.layout.Vpad, teacher_logits, uncond_logits, ldt, sh.V, a["lse_rows"], teacher_lse, uncond_lse,
                        scale, B, sh.P, L, float(B if batch_den is None else batch_den), row, lg, smp, kd)
        a.update(kd_row=row, kd_lg=lg, kd_sample=smp, kd=kd,
                 kd_teacher=(teacher_logits, uncond_logits, ldt, teacher_lse, uncond_lse, float(scale)))
        return kd

    def loss_backward_kd(self, gscale=1.0, lm_coef=0.0, kd_coef=0.0):
        """loss_backward() with kd_coef * d(sum of the row terms)/d logits added, kd_coef = distill_weight * gscale / (ntok *
        batch_den); the same buffers and storage forms.  Reads the teacher tensors distill_loss() was given."""
        a, sh = self.act, self.sh
        if "kd_lg" not in a:
            raise RuntimeError("loss_backward_kd() needs distill_loss() on this forward")
        Vp = self.layout.Vpad
        cond, uncond, ldt, lse_c, lse_u, scale = a["kd_teacher"]
        args = (a["logits"], Vp, sh.V, a["topic_ids"], a["targets"], a["lse_rows"], a["coef"], gscale, cond, uncond, ldt, lse_c, lse_u,
                scale, a["kd_lg"], kd_coef, a["B"], sh.P, a["L"])
        if a.get("x3") and self.hybrid:
            dl = self.buf("dlogits_b", (a["M"], Vp), torch.bfloat16)
            hip.loss_bwd_kd(*args, dl, Vp, Vp, lm_coef=lm_coef)
            return dl
        if a.get("x3"):
            dlp = self.pbuf("dlogits_p", a["M"], Vp)
            hip.loss_bwd_kd_x3(*args, dlp, Vp, lm_coef=lm_coef)
            return dlp
        dl = a["logits"] if a["logits"].dtype == self.tdt and self.dtype != hip.F32 else self.buf("dlogits", (a["M"], Vp))
        hip.loss_bwd_kd(*args, dl, Vp, Vp, lm_coef=lm_coef)
        return dl

    def dlogits_from(self, g32):
        """External d(logits) [B,T,V] fp32 (drop-in autograd path) -> padded compute-dtype buffer."""
        a = self.act
        dl = self.buf("dlogits_b", (a["M"], self.layout.Vpad), torch.bfloat16) if (self.hybrid and a.get("x3")) else self.buf("dlogits", (a["M"], self.layout.Vpad))
        g32 = g32.contiguous().view(a["M"], self.sh.V)
        hip.cast_pad_rows(g32, self.sh.V, dl, self.layout.Vpad, a["M"], self.sh.V)
        return dl

    # ---------------------------------------------------------------- backward
    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        return self._side

    def _event(self, i):
        ev = self._events.get(i)
        if ev is None:
            ev = self._events[i] = torch.cuda.Event()
        return ev

    def _ready(self, pack):
        if self.bucket_hook is not None:
            self._flush_sums()          # the gradients the hook may hand to the exchange must be final: pending column sums first
            self.bucket_hook(pack)

    # ---- deferred column sums (mmtg_colsum_batch): the sources are per-site workspaces that nothing rewrites before the flush
    def _defer_sum(self, X, ldx, M, N, out, offset=0):
        """out[c] += sum_{r < M} X[offset + r * ldx + c], c < N, at the next flush (fp32 X, M <= 2048)."""
        self._sums.append((X.data_ptr() + 4 * offset, out.data_ptr(), int(ldx), int(M), int(N)))

    def _flush_sums(self):
        if self._sums:
            # the items of a flush run concurrently: no two may add into the same output elements
            spans = sorted((it[1], it[1] + 4 * it[4]) for it in self._sums)
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                if b0 < a1:
                    raise RuntimeError("deferred column sums with overlapping outputs in one batch")
            hip.colsum_batch(self._sums)
            self._sums = []

    def _ln_bwd_x3(self, site, dy, x, gamma_key, mean, rstd, dres, dx, rows, cols, dx_planes, drop_p=0.0, drop_seed=0, colsum_key=None):
        """_ln_bwd for the split-precision path (fp32 rows, the masked gradient written as a plane pair)."""
        g = gamma_key[:-len("weight")]
        if self._defer:
            ws = self.buf("ln_bwd_ws_" + site, (hip.lib().mmtg_layernorm_bwd_ws(rows, cols),), torch.float32)
            nb = hip.layernorm_bwd_x3_partial(dy, x, self.P(gamma_key), mean, rstd, dres, dx, rows, cols, dx_planes, ws,
                                              drop_p=drop_p, drop_seed=drop_seed, want_colsum=colsum_key is not None)
            self._defer_sum(ws, 3 * cols, nb, cols, self.G(gamma_key))
            self._defer_sum(ws, 3 * cols, nb, cols, self.G(g + "bias"), offset=cols)
            if colsum_key is not None:
                self._defer_sum(ws, 3 * cols, nb, cols, self.G(colsum_key), offset=2 * cols)
        else:
            lnws = self.buf("ln_bwd_ws", (hip.lib().mmtg_layernorm_bwd_ws(rows, max(self.sh.D, self.sh.H)),), torch.float32)
            hip.layernorm_bwd_x3(dy, x, self.P(gamma_key), mean, rstd, dres, dx, self.G(gamma_key), self.G(g + "bias"), rows, cols, dx_planes,
                                 drop_p=drop_p, drop_seed=drop_seed, dcolsum=None if colsum_key is None else self.G(colsum_key), ws=lnws)

    def _ln_bwd(self, site, dy, x, gamma_key, mean, rstd, dres, dx, rows, cols, dx_masked=None, drop_p=0.0, drop_seed=0, colsum_key=None):
        """LayerNorm backward of the bf16 decoder path: with deferred sums the first stage only, into this site's own partial-row
        workspace, the three gradients it ends in queued for the batched sum; otherwise the one-call form on the shared workspace."""
        g = gamma_key[:-len("weight")]
        if self._defer:
            ws = self.buf("ln_bwd_ws_" + site, (hip.lib().mmtg_layernorm_bwd_ws(rows, cols),), torch.float32)
            nb = hip.layernorm_bwd_partial(dy, x, self.P(gamma_key), mean, rstd, dres, dx, rows, cols, ws, dx_masked=dx_masked,
                                           drop_p=drop_p, drop_seed=drop_seed, want_colsum=colsum_key is not None)
            self._defer_sum(ws, 3 * cols, nb, cols, self.G(gamma_key))
            self._defer_sum(ws, 3 * cols, nb, cols, self.G(g + "bias"), offset=cols)
            if colsum_key is not None:
                self._defer_sum(ws, 3 * cols, nb, cols, self.G(colsum_key), offset=2 * cols)
        else:
            lnws = self.buf("ln_bwd_ws", (hip.lib().mmtg_layernorm_bwd_ws(rows, max(self.sh.D, self.sh.H)),), torch.float32)
            hip.layernorm_bwd(dy, x, self.P(gamma_key), mean, rstd, dres, dx, self.G(gamma_key), self.G(g + "bias"), rows, cols,
                              dx_masked=dx_masked, drop_p=drop_p, drop_seed=drop_seed,
                              dcolsum=None if colsum_key is None else self.G(colsum_key), ws=lnws)

    @contextlib.contextmanager
    def _as_bf16(self):
        """The decoder part of the hybrid mode's backward runs the bf16 mode's code path on an fp32-storage engine: for its
        duration the engine presents bf16 storage -- buffers default to bf16, W() / Wt() / the [D, Vpad] copy are the HI planes of
        the weight plane pairs (hi = bf16(w): the bf16 mode's own weight copy, bit for bit)."""
        saved = (self.dtype, self.tdt, self.x3, self.wc, self.wt, self.wte_t)
        self.dtype, self.tdt, self.x3 = hip.BF16, torch.bfloat16, False
        self.wc = self.wc2[0]
        self.wt = None if saved[4] is None else saved[4][0]
        self.wte_t = None if saved[5] is None else saved[5][0]
        try:
            yield
        finally:
            self.dtype, self.tdt, self.x3, self.wc, self.wt, self.wte_t = saved

    def _backward_hybrid(self, dlogits, dkl, cl=None):
        """compute_dtype "bf16x3f": d(logits) through the decoder as ONE bf16 pass per product -- the bf16 mode's kernels over the hi
        planes the split-precision forward stored (LayerNorm outputs, qkv, attention context, GELU output, projector activations),
        the bf16 copies of the LayerNorm inputs and of the c_fc pre-activation it wrote beside them, and the hi planes of the
        weights -- then the encoder / fuser backward, on the bf16 kernels as well.  Gradients land in the same flat fp32 buffer."""
        a, sh = self.act, self.sh
        M, Vp = a["M"], self.layout.Vpad
        if isinstance(dlogits, hip.Planes):
            dlogits = dlogits.t[0]
        if dlogits.dtype != torch.bfloat16:
            dlb = self.buf("dlogits_b", (M, Vp), torch.bfloat16)
            hip.cast_f32_to(dlogits, dlb, M * Vp)
            dlogits = dlb
        hi = lambda pl: pl.t[0]
        layers = []
        for rec, (xb1, xb2) in zip(a["layers"], a["hyb_rows"]):
            (xin, mu1, rs1, a1, qkv, ctx, lse, xmid, mu2, rs2, m2, u, gact, s_, ctxp) = rec
            layers.append((xb1, mu1, rs1, hi(a1), hi(qkv), hi(ctxp), lse, xb2, mu2, rs2, hi(m2), u, hi(gact), s_, None))
        ab = dict(a)
        if a.get("px3"):
            h1b, xb = hi(a["h1p"]), hi(a["xp"])
        else:       # (projector widths the split-precision products do not tile: fp32 rows, cast once)
            h1b = self.buf("h1_b", tuple(a["h1"].shape), torch.bfloat16)
            hip.cast_f32_to(a["h1"], h1b, a["h1"].numel())
            xb = self.buf("x_cond_b", tuple(a["x"].shape), torch.bfloat16)
            hip.cast_f32_to(a["x"], xb, a["x"].numel())
        ab.update(x3=False, px3=False, elem_mask=True, layers=layers, x_last=a["x_last_b"], hf=hi(a["hf"]), h1=h1b, x=xb, ids32=None)
        try:
            with self._as_bf16():
                self.act = ab
                seg = self._backward_decoder(ab, dlogits, cl)
        finally:
            self.act = a
        # the encoder / fuser backward on the bf16 kernels too (the mode's gradients are bf16-accurate by contract): bf16 copies of
        # the ~14 small activations it reads (320 x 512 ... 320 x 2048), then the same code path under the bf16 presentation --
        # 0.8 ms of exact-fp32 products (14 TFLOP/s on 34 few-row launches) become ~0.2
        ae = self._encoder_record_bf16(a)
        with self._as_bf16():
            self._backward_encoder(ae, seg, dkl)

    def _encoder_record_bf16(self, a):
        """The activation record `_backward_encoder` reads, with every fp32 tensor it takes as a kernel operand replaced by a bf16
        copy (statistics, attention probabilities, cell saves and fuser weights stay fp32: the bf16 kernels read them as fp32 too)."""
        def cast(t, name):
            b = self.buf("hyb_" + name, tuple(t.shape), torch.bfloat16)
            hip.cast_f32_to(t, b, t.numel())
            return b
        ae = dict(a)
        for k in ("o", "t_ln", "t_raw", "xt"):
            ae[k] = cast(a[k], k)
        ae["alpha"] = {mod: (cast(q, "aqkv_" + mod), cast(c, "actx_" + mod), p) for mod, (q, c, p) in a["alpha"].items()}
        enc = {}
        for ch, (layers, h_ln) in a["enc"].items():
            recs = []
            for l, rec in enumerate(layers):
                r = dict(rec)
                r["h"] = cast(rec["h"], "h_%s%d" % (ch, l))
                r["inp"] = recs[l - 1]["h"] if (l > 0 and rec["inp"] is layers[l - 1]["h"]) else cast(rec["inp"], "inp_%s%d" % (ch, l))
                recs.append(r)
            enc[ch] = (recs, cast(h_ln, "hln_" + ch))
        ae["enc"] = enc
        return ae

    def backward(self, dlogits, dkl=0.0, cl_coef=0.0, cl_margin=None):
        """Back-propagate d(logits) [M,Vpad] (compute dtype) and d(kl) through the whole
        model; parameter gradients are ACCUMULATED into the flat fp32 buffer.
        cl_coef > 0 (after cl_loss() on this forward): cl_coef * d(sum_b cl_sample)/d(hf) is added to d(ln_f output) between the LM
        head and ln_f's backward, cl_coef = cl_weight * gscale / batch_den; cl_margin: None = the margin cl_loss() used."""
        a = self.act
        cl = self._cl_record(a, cl_coef, cl_margin) if cl_coef > 0.0 else None
        self.ensure_grad()
        # (nothing of an earlier backward that raised may reach this one: its queued column sums hold raw pointers)
        self._sums, self._defer, self._tail_jobs = [], False, []
        try:
            if self._lazy is not None and not self.wgrad_overwrite:
                # (a backward that accumulates after a zero_grad(shape_key) that relied on overwrites: zero what it skipped)
                self.grad.zero_()
                self._lazy = None
            if self.hybrid and a.get("x3"):
                self._backward_hybrid(dlogits, dkl, cl)
            else:
                self._backward_encoder(a, self._backward_decoder(a, dlogits, cl), dkl)
        finally:
            # (on the way out of an exception too: a window of micro-batches would otherwise accumulate on top of what is left)
            if self._tail_side is not None:         # the weight gradients that ran beside the tail: final before anything reads the gradient
                torch.cuda.current_stream().wait_stream(self._tail_side)
                self._tail_side = None
            self._sums, self._defer, self._tail_jobs = [], False, []
            self._lazy = None

    def _backward_decoder(self, a, dlogits, cl=None):
        """LM head -> GPT-2 blocks -> input embedding -> projector; returns the per-segment sums of d(h1_pre) [B*S, H] that the
        experience vectors' gradient is made of.  cl: backward()'s record of the contrastive term, or None."""
        dhf = self._bwd_lm_head(a, dlogits)
        if cl is not None:
            # (the LM head's side-stream weight gradient reads dlogits and hf only: d_hf is this stream's own)
            hf, rinv, margin, coef = cl
            hip.cl_bwd(hf, self.sh.D, a["keep"], self.sh.P + a["L"], rinv, margin, coef, a["B"], self.sh.P, a["L"], self.sh.D, dhf, self.sh.D)
        dx = self._bwd_blocks(a, dhf)
        # (deferred column sums: everything the blocks queued since the last hand-over point -- the whole decoder's without a bucket hook --
        #  in one launch, here, with the embedding / projector / encoder backward still to come behind it)
        self._flush_sums()
        self._defer = False
        # (the side stream forks here, beside the embedding / projector backward too: 14.28 -> 14.10 ms against a fork after the projector)
        self._launch_tail_jobs()
        return self._bwd_embed_projector(a, dx)

    # ---- grouped weight-gradient launches (mmtg_wgrad_group): sizing and launch
    def _group_bufs(self, shapes, cfg, rule, ws_name, cnt_name="wgrad_group_cnt"):
        """(splits, workspace, counters) of a grouped launch: _group_sizing's numbers, the named workspace (none for one split)
        and the named counter tensor."""
        splits, nws, ncnt = _group_sizing(shapes, cfg, rule)
        ws = self.buf(ws_name, (nws,), torch.float32) if splits > 1 else None
        cnt = self.ws.get((cnt_name, torch.int32))
        if cnt is None or cnt.numel() < ncnt:      # zero once: every launch leaves the counters zeroed
            cnt = self.ws[(cnt_name, torch.int32)] = torch.zeros(ncnt, device=self.dev, dtype=torch.int32)
        return splits, ws, cnt

    def _launch_group(self, probs, M, bufs, cfg, written, side=None, event=None, tail=False):
        """One grouped launch over `bufs` (_group_bufs): on the current stream, on `side` behind everything enqueued so far (`event`
        recorded after it), or queued for the backward's tail.  `written`: the (offset, count) gradient ranges it writes, for the
        record the lazy zero_grad is built from."""
        splits, ws, cnt = bufs
        if tail:
            self._tail_jobs.append((probs, M, splits, ws, cnt, not self.wgrad_overwrite, cfg))       # launched at the tail
        elif side is not None:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                hip.wgrad_group(probs, M, splits, ws, cnt, accumulate=not self.wgrad_overwrite, config=cfg)
                if event is not None:
                    event.record(side)
        else:
            hip.wgrad_group(probs, M, splits, ws, cnt, accumulate=not self.wgrad_overwrite, config=cfg)
        if self.wgrad_overwrite and self._ow_rec is not None:
            self._ow_rec[1].extend(written)

    # ---- stage 1: LM head (tied wte)
    def _bwd_lm_head(self, a, dlogits):
        """d(ln_f output) = dlogits wte into d_hf (returned), and the tied embedding's weight gradient dlogits^T hf."""
        M, D, Vp = a["M"], self.sh.D, self.layout.Vpad
        pr = a["pdrop"][2]
        dhf = self.buf("d_hf", (M, D))
        x3 = bool(a.get("x3"))
        if x3:
            # split-precision backward: d(logits) as a plane pair feeds both the LM head's dgrad (through the [D, Vpad] copy of the
            # tied embedding) and its weight gradient (grouped kernel: written, not accumulated with atomics)
            dlp = dlogits if isinstance(dlogits, hip.Planes) else hip.split_planes(dlogits, M, Vp, self.pbuf("dlogits_p", M, Vp))
            hip.gemm_x3(dlp, hip.Planes(self.wte_t, D, Vp), dhf, M, D, Vp)
        elif self.wte_t is not None and Vp % 128 == 0 and not self.x3:      # (x3: wte_t is a plane pair)
            hip.gemm(dlogits, self.wte_t, dhf, M, D, Vp, transB=True, ldb=Vp)
        else:
            hip.gemm(dlogits, self.Wp("wte"), dhf, M, D, Vp, transB=False, ldb=D)
        # (Vpad rows: the pad columns of dlogits are zero, so the pad rows of the pack receive +0)
        wte = [(self.layout.pack_range["wte"][0], Vp * D)]
        if x3:
            bufs = self._group_bufs(((Vp, D),), 0, lambda tiles: _LMHEAD_GROUP_SPLITS or _group_splits_x3(tiles, M), "wgrad_group_ws_head")
            self._launch_group([(dlp, a["hf"], self.Gp("wte"), Vp, D, Vp, D, D)], M, bufs, _X3_WG_CFG, wte)
        elif self.dtype == hip.BF16 and M >= 256 and D % 8 == 0 and Vp % 8 == 0:
            # the tied embedding's gradient through the grouped kernel too: no fp32 atomics (bit-reproducible), and the
            # gradient is WRITTEN, so the lazy zero_grad can skip its 41 MB (the type-embedding rows are added later)
            hcfg = hip.WGRAD_RING if _group_cfg(D) == hip.WGRAD_RING else 0      # (the ring form: the same rule on its 256 slots)
            # (a workspace of its own: under MMTG_WGRAD_STREAM this launch may still be pending on the side stream when the
            #  block launches size theirs -- a shared name could reallocate, i.e. free, the buffer under it)
            bufs = self._group_bufs(((Vp, D),), hcfg, lambda tiles: _LMHEAD_GROUP_SPLITS or _group_splits(tiles, M, 256 if hcfg else 1024),
                                    "wgrad_group_ws_head")
            # (MMTG_WGRAD_STREAM: beside the LM head's dgrad, ln_f and the last block's chain -- reads dlogits / hf only)
            self._launch_group([(dlogits, a["hf"], self.Gp("wte"), Vp, D, Vp, D, D)], M, bufs, hcfg, wte,
                               side=self._side_stream() if (_WGRAD_STREAM and pr > 0) else None)
        else:
            splits = _wgrad_splits(Vp, D, M, self.dtype == hip.BF16)
            if self.dtype == hip.F32 and not self.x3 and splits > 1:
                # exact-fp32 mode: K-split slabs summed in order ON TOP of what the gradient already holds (no fp32 atomics)
                part = self.buf("wgrad_slabs", (splits * Vp * D,), torch.float32)
                hip.gemm(dlogits, a["hf"], part, Vp, D, M, transA=True, transB=False, lda=Vp, ldb=D, ldc=D,
                         epi=hip.EPI_SPLIT, out_f32=True, splits=splits)
                hip.slab_sum(part, splits, Vp * D, self.Gp("wte"), Vp * D, accumulate=True)
            else:
                hip.gemm(dlogits, a["hf"], self.Gp("wte"), Vp, D, M, transA=True, transB=False, lda=Vp, ldb=D, ldc=D,
                         epi=hip.EPI_ATOMIC, splits=splits)
        return dhf

    # ---- stage 2: ln_f and the GPT-2 blocks
    def _bwd_blocks(self, a, dhf):
        """ln_f and the blocks, top to bottom; owns the gradient buffers the chain runs through -- one shared set, a set per block
        parity under MMTG_WGRAD_STREAM, a set per deferred block under MMTG_WGRAD_TAIL.  Returns d(resid_0), the input embedding's
        gradient.  Every LayerNorm backward on the residual stream also emits, in the same pass, the dropout-masked gradient
        entering the previous residual branch and that branch's bias gradient (column sum) -- see mmtg_layernorm_bwd."""
        sh = self.sh
        B, T, M, D = a["B"], a["T"], a["M"], sh.D
        pr = a["pdrop"][2]
        pre = "decoder.gpt2.transformer."
        x3 = bool(a.get("x3"))
        self._defer = _DEFER_SUMS and (self.dtype == hip.BF16 or x3)
        s = SimpleNamespace(dx=self.buf("d_resid_a", (M, D)), dx2=self.buf("d_resid_b", (M, D)))
        # One grouped launch per block for its four weight gradients (mmtg_wgrad_group): the mlp.c_proj product's dy must then
        # outlive the LayerNorm backward that produces the attention c_proj's dy, so the masked gradients alternate
        # between two buffers.
        group = s.group = (self.dtype == hip.BF16 and M >= 256 and D % 8 == 0) or x3
        s.dmask = self.buf("d_masked", (M, D)) if (pr > 0 and not x3) else None
        s.dmask_b = (self.buf("d_masked_b", (M, D)) if group else s.dmask) if (pr > 0 and not x3) else None
        if group:
            gcfg = _group_cfg(D, x3)
            rule = (lambda tiles: _group_splits_x3(tiles, M)) if x3 else (lambda tiles: _group_splits(tiles, M, 256 if gcfg else 1024))
            s.gbufs = self._group_bufs(((D, 4 * D), (4 * D, D), (D, D), (D, 3 * D)), gcfg, rule, "wgrad_group_ws")
            s.gcfg = _X3_WG_CFG if x3 else gcfg
        lastp = f"{pre}h.{sh.L - 1}."
        # (MMTG_WGRAD_STREAM: the top block's masked gradient goes into the buffer set of that block's parity, see below)
        dmask_top = self.buf("d_masked_1", (M, D)) if (group and not x3 and _WGRAD_STREAM and pr > 0 and (sh.L - 1) & 1) else s.dmask
        # MMTG_WGRAD_TAIL: the last blocks' operand buffers are their own (nothing rewrites them before their launch at the tail)
        # (the split-precision blocks' operands are plane pairs the LayerNorm backward writes with or without dropout: name suffix per block)
        ntail = s.ntail = min(_WGRAD_TAIL, sh.L) if (group and not _WGRAD_STREAM and (pr > 0 or x3) and self.bucket_hook is None) else 0
        s.tsets = {} if x3 else {t: (self.buf("d_u_t%d" % t, (M, 4 * D)), self.buf("d_masked_t%d" % t, (M, D)),
                                     self.buf("d_masked_b_t%d" % t, (M, D)), self.buf("d_qkv_t%d" % t, (M, 3 * D))) for t in range(ntail)}
        s.xsfx = (lambda t: "_t%d" % t if t < ntail else "") if x3 else (lambda t: "")
        if ntail == sh.L and not x3:
            dmask_top = s.tsets[sh.L - 1][1]
        self._tail_jobs = []
        if x3:
            # (x3: every LayerNorm backward writes the masked gradient entering the previous residual branch as the plane pair
            #  that branch's split-precision products read -- no fp32 copy, no separate split pass)
            s.dyp = self.pbuf("d_masked_p" + s.xsfx(sh.L - 1), M, D)
            self._ln_bwd_x3("f", dhf, a["x_last"], pre + "ln_f.weight", a["muf"], a["rsf"], None, s.dx, M, D, s.dyp,
                            drop_p=pr, drop_seed=a["layers"][sh.L - 1][13][2], colsum_key=lastp + "mlp.c_proj.bias")
        else:
            self._ln_bwd("f", dhf, a["x_last"], pre + "ln_f.weight", a["muf"], a["rsf"], None, s.dx, M, D,
                         dx_masked=dmask_top, drop_p=pr, drop_seed=a["layers"][sh.L - 1][13][2], colsum_key=lastp + "mlp.c_proj.bias")
        self._ready("ln_f.b")
        s.du = None if x3 else self.buf("d_u", (M, 4 * D))
        s.dm = self.buf("d_m", (M, D))
        s.dctx = self.buf("d_ctx", (M, D))
        s.dqkv = self.buf("d_qkv", (M, 3 * D))
        # MMTG_WGRAD_STREAM: block l's grouped weight gradients run on a side stream while the main stream already walks block
        # l - 1 -- the operands the chain produces (du, the two masked residual gradients, dqkv) then live in two buffer sets that
        # alternate block by block, and the main stream waits for block l + 1's launch before it rewrites that block's set.
        s.stream_mode = group and _WGRAD_STREAM and pr > 0 and not x3
        if s.stream_mode:
            s.side = self._side_stream()
            odd = (self.buf("d_u_1", (M, 4 * D)), self.buf("d_masked_1", (M, D)), self.buf("d_masked_b_1", (M, D)),
                   self.buf("d_qkv_1", (M, 3 * D)))
            s.sets = ((s.du, s.dmask, s.dmask_b, s.dqkv), odd)
            s.wdone = {}
        s.da = self.buf("d_a", (M, D))
        s.delta = self.buf("attn_delta", (M, sh.nH), torch.float32)
        # (x3: one [M, D] buffer per block of 128 keys -- plain stores summed in block order, no atomics)
        s.dq32 = self.buf("attn_dq32", (hip.attn_bwd_x3_dq_floats(B, T, D),) if x3 else (M, D), torch.float32)
        block = self._bwd_block_x3 if x3 else self._bwd_block
        for l in range(sh.L - 1, -1, -1):
            if s.stream_mode:
                s.du, s.dmask, s.dmask_b, s.dqkv = s.sets[l & 1]
            if l in s.tsets:
                s.du, s.dmask, s.dmask_b, s.dqkv = s.tsets[l]
            block(a, l, s)
        if s.stream_mode:
            torch.cuda.current_stream().wait_stream(s.side)        # block 0's launch (and the tied embedding's, long done)
            for l_ in sorted(s.wdone, reverse=True):
                self._ready(f"{pre}h.{l_}.ln_1.bias")
        elif _WGRAD_STREAM and pr > 0 and self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)  # (only the tied embedding's gradient ran on the side stream)
        return s.dx

    def _bwd_block_x3(self, a, l, s):
        """Split-precision backward of block l: every gradient that feeds a product travels as a plane pair.  In: s.dx = d(block
        output), s.dyp = its masked planes; out: s.dx = d(block input), s.dyp = the planes block l - 1 reads."""
        sh = self.sh
        B, T, M, D = a["B"], a["T"], a["M"], sh.D
        _, pa, pr = a["pdrop"]
        pre = "decoder.gpt2.transformer."
        p = f"{pre}h.{l}."
        dx, dx2, dm, da, delta, dq32, dyp = s.dx, s.dx2, s.dm, s.da, s.delta, s.dq32, s.dyp
        (xin, mu1, rs1, a1, qkv, ctx, lse, xmid, mu2, rs2, m2, u, gact, seeds, ctxp) = a["layers"][l]
        bands = self.buf("d_u_bands_%d" % l if self._defer else "d_u_bands", ((M + 63) // 64, 4 * D), torch.float32)
        dup = self.pbuf("d_u_p" + s.xsfx(l), M, 4 * D)
        self._dgrad_x3(dyp, p + "mlp.c_proj.weight", None, M, planes=dup, ldc=4 * D, epi=hip.EPI_DGELU, aux=u, ldaux=4 * D, aux2=bands)
        if self._defer and bands.shape[0] <= 2048:
            self._defer_sum(bands, 4 * D, bands.shape[0], 4 * D, self.G(p + "mlp.c_fc.bias"))
        else:
            hip.colsum(bands, bands.shape[0], 4 * D, self.G(p + "mlp.c_fc.bias"))
        self._dgrad_x3(dup, p + "mlp.c_fc.weight", dm, M)
        dy2p = self.pbuf("d_masked_b_p" + s.xsfx(l), M, D)
        self._ln_bwd_x3("%d_2" % l, dm, xmid, p + "ln_2.weight", mu2, rs2, dx, dx2, M, D, dy2p,
                        drop_p=pr, drop_seed=seeds[1], colsum_key=p + "attn.c_proj.bias")
        dqkvp = self.pbuf("d_qkv_p" + s.xsfx(l), M, 3 * D)
        # d(ctx) as a plane pair only (the attention backward is its one reader); the dgrad's epilogue also emits delta =
        # rowsum(d ctx * ctx) per head: no separate pass over ctx / d ctx
        dctxp = self.pbuf("d_ctx_p", M, D)
        self._dgrad_x3(dy2p, p + "attn.c_proj.weight", None, M, planes=dctxp, ldc=D, epi=hip.EPI_ROWDOT, aux=ctx, ldaux=D, aux2=delta)
        # (deferred sums: the partial bias rows -- k / v parts per key block, q part per 16-row band -- stay in this block's own scratch)
        nkv, nq = B * (-(-T // 128)), -(-M // 16)
        brows = self._defer and nkv <= 2048 and nq <= 2048
        bws = self.buf("attn_dbias_x3_%d" % l if brows else "attn_dbias_x3", (hip.attn_bwd_x3_ws(B, T, D),), torch.float32)
        hip.attn_bwd_x3(qkv, a["keep"], ctx, dctxp, lse, delta, dq32, dqkvp, B, T, sh.nH, D // sh.nH, drop_p=pa, drop_seed=seeds[0],
                        dbias=None if brows else self.G(p + "attn.c_attn.bias"), delta_ready=True, dbias_ws=bws)
        if brows:
            # (two items must not share output columns -- they run in one launch: the key-block rows carry the k and v parts,
            #  their q columns are zero; the band rows carry the q part)
            self._defer_sum(bws, 3 * D, nkv, 2 * D, self.G(p + "attn.c_attn.bias")[D:], offset=D)
            self._defer_sum(bws, D, nq, D, self.G(p + "attn.c_attn.bias"), offset=nkv * 3 * D)
        self._dgrad_x3(dqkvp, p + "attn.c_attn.weight", da, M)
        keys = (p + "mlp.c_fc.weight", p + "mlp.c_proj.weight", p + "attn.c_proj.weight", p + "attn.c_attn.weight")
        probs = [(m2, dup, self.G(keys[0]), D, 4 * D), (gact, dyp, self.G(keys[1]), 4 * D, D),
                 (ctxp, dy2p, self.G(keys[2]), D, D), (a1, dqkvp, self.G(keys[3]), D, 3 * D)]
        written = ((self.layout.entries[k][0], self.layout.entries[k][2]) for k in keys)
        self._launch_group(probs, M, s.gbufs, s.gcfg, written, tail=l < s.ntail)
        if l > 0:
            s.dyp = self.pbuf("d_masked_p" + s.xsfx(l - 1), M, D)          # the planes block l - 1 reads (its own when it is deferred)
            self._ln_bwd_x3("%d_1" % l, da, xin, p + "ln_1.weight", mu1, rs1, dx2, dx, M, D, s.dyp,
                            drop_p=pr, drop_seed=a["layers"][l - 1][13][2], colsum_key=f"{pre}h.{l - 1}.mlp.c_proj.bias")
        else:
            self._ln_bwd("0_1", da, xin, p + "ln_1.weight", mu1, rs1, dx2, dx, M, D)
        self._ready(p + "ln_1.bias")

    def _bwd_block(self, a, l, s):
        """bf16 / exact-fp32 backward of block l.  In: s.dx = d(block output), s.dmask = its dropout-masked copy; out: s.dx =
        d(block input), the masked copy in the set block l - 1 reads."""
        sh = self.sh
        B, T, M, D = a["B"], a["T"], a["M"], sh.D
        _, pa, pr = a["pdrop"]
        pre = "decoder.gpt2.transformer."
        p = f"{pre}h.{l}."
        dx, dx2, dm, dctx, da, delta, dq32 = s.dx, s.dx2, s.dm, s.dctx, s.da, s.delta, s.dq32
        du, dmask, dmask_b, dqkv = s.du, s.dmask, s.dmask_b, s.dqkv
        group, stream_mode = s.group, s.stream_mode
        (xin, mu1, rs1, a1, qkv, ctx, lse, xmid, mu2, rs2, m2, u, gact, seeds, ctxp) = a["layers"][l]
        # x_out = x_mid + drop(gact W2 + b2): dy = dx * mask (already produced, with its bias gradient)
        dy = dmask if pr > 0 else dx
        # (the dGELU epilogue also emits the column sums of du per 64-row band: a [M/64, 4D] reduction
        #  gives the c_fc bias gradient instead of a pass over du)
        bands = self.buf("d_u_bands_%d" % l if self._defer else "d_u_bands", ((M + 63) // 64, 4 * D), torch.float32)
        self._dgrad(dy, p + "mlp.c_proj.weight", du, M, "conv1d", epi=hip.EPI_DGELU, aux=u, ldaux=4 * D, aux2=bands)
        if self._defer and bands.shape[0] <= 2048:
            self._defer_sum(bands, 4 * D, bands.shape[0], 4 * D, self.G(p + "mlp.c_fc.bias"))
        else:
            hip.colsum(bands, bands.shape[0], 4 * D, self.G(p + "mlp.c_fc.bias"))
        # (both consumers of du run while it is still in the Infinity Cache; the c_proj weight gradient, whose
        #  operands come from HBM either way, goes last -- it must precede the LayerNorm backward, which reuses dmask)
        self._dgrad(du, p + "mlp.c_fc.weight", dm, M, "conv1d")
        dy_fc2 = dy
        if not group:
            self._wgrad(m2, du, p + "mlp.c_fc.weight", None, M, "conv1d")
            self._wgrad(gact, dy, p + "mlp.c_proj.weight", None, M, "conv1d")
        self._ln_bwd("%d_2" % l, dm, xmid, p + "ln_2.weight", mu2, rs2, dx, dx2, M, D,
                     dx_masked=dmask_b, drop_p=pr, drop_seed=seeds[1], colsum_key=p + "attn.c_proj.bias")
        # x_mid = x_in + drop(ctx Wp + bp)
        dy = dmask_b if pr > 0 else dx2
        # bf16: the dgrad GEMM's epilogue also emits delta = rowsum(d ctx * ctx) per head
        fuse_delta = self.dtype == hip.BF16 and M > 256
        if fuse_delta:
            self._dgrad(dy, p + "attn.c_proj.weight", dctx, M, "conv1d", epi=hip.EPI_ROWDOT, aux=ctx, ldaux=D, aux2=delta)
        else:
            self._dgrad(dy, p + "attn.c_proj.weight", dctx, M, "conv1d")
        if not group:
            self._wgrad(ctx, dy, p + "attn.c_proj.weight", None, M, "conv1d")
        # (hybrid: the split-precision forward drew the attention-dropout mask element by element; the whole-head backward
        #  kernels regenerate THAT mask instead of their own word masks)
        # (exact-fp32 mode: the tiled kernel combines its waves' bias sums with LDS atomics -- arrival order -- so the c_attn bias
        #  gradient is an ordered column sum over d(qkv) there instead: one more pass in the cross-check mode, reproducible bits)
        exact = self.dtype == hip.F32 and not self.x3
        # (deferred sums: the whole-head kernels leave their B partial bias rows in this block's own scratch for the batched sum)
        brows = hip.attn_bwd_dbias_rows(self.dtype, B, T) if self._defer else 0
        brows = brows if 0 < brows <= 2048 else 0
        bws = None if exact else self.buf("attn_dbias_rows_%d" % l if brows else "attn_dbias_rows",
                                           (hip.attn_bwd_bias_rows(B, T, self.dtype), 3 * D), torch.float32)
        hip.attn_bwd(qkv, a["keep"], ctx, dctx, lse, delta, dq32, dqkv, B, T, sh.nH, D // sh.nH,
                     drop_p=pa, drop_seed=seeds[0], delta_ready=fuse_delta, dbias=None if exact else self.G(p + "attn.c_attn.bias"),
                     flags=(hip.ATTN_ELEM_MASK if a.get("elem_mask") else 0) | (hip.ATTN_DBIAS_ROWS if brows else 0), dbias_ws=bws)
        if brows:
            self._defer_sum(bws, 3 * D, brows, 3 * D, self.G(p + "attn.c_attn.bias"))
        if exact:
            hip.colsum(dqkv, M, 3 * D, self.G(p + "attn.c_attn.bias"))
        self._dgrad(dqkv, p + "attn.c_attn.weight", da, M, "conv1d")
        if group:
            # gw[in, out] (+)= x^T dy for the block's four Conv1D layers: 432 tiles x 2 K halves at GPT-2 base, reduced in
            # the kernel (must run before the LayerNorm backward below, which rewrites dmask / dx for the next block)
            keys = (p + "mlp.c_fc.weight", p + "mlp.c_proj.weight", p + "attn.c_proj.weight", p + "attn.c_attn.weight")
            probs = [(m2, du, self.G(keys[0]), D, 4 * D), (gact, dy_fc2, self.G(keys[1]), 4 * D, D),
                     (ctx, dy, self.G(keys[2]), D, D), (a1, dqkv, self.G(keys[3]), D, 3 * D)]
            written = ((self.layout.entries[k][0], self.layout.entries[k][2]) for k in keys)
            if stream_mode:
                s.wdone[l] = self._event(l)
                self._launch_group(probs, M, s.gbufs, s.gcfg, written, side=s.side, event=s.wdone[l])
            else:
                self._launch_group(probs, M, s.gbufs, s.gcfg, written, tail=l in s.tsets)
        else:
            self._wgrad(a1, dqkv, p + "attn.c_attn.weight", None, M, "conv1d")
        if stream_mode and (l + 1) in s.wdone:
            # block l + 1's weight gradients have read the set this LayerNorm backward starts to rewrite; its gradients are
            # final only now (the data-parallel bucket hook must not see them earlier)
            torch.cuda.current_stream().wait_event(s.wdone.pop(l + 1))
            self._ready(f"{pre}h.{l + 1}.ln_1.bias")
        if l > 0:
            self._ln_bwd("%d_1" % l, da, xin, p + "ln_1.weight", mu1, rs1, dx2, dx, M, D,
                         dx_masked=(s.sets[(l - 1) & 1][1] if stream_mode else s.tsets[l - 1][1] if (l - 1) in s.tsets else dmask),
                         drop_p=pr, drop_seed=a["layers"][l - 1][13][2],
                         colsum_key=f"{pre}h.{l - 1}.mlp.c_proj.bias")
        else:
            self._ln_bwd("0_1", da, xin, p + "ln_1.weight", mu1, rs1, dx2, dx, M, D)
        if not stream_mode:
            self._ready(p + "ln_1.bias")

    # ---- stage 3: input embedding and projector
    def _bwd_embed_projector(self, a, dx):
        """GPT-2 input embedding h0 = drop(g + wpe + wte[type]) and the projector (model.py:279-281); returns the per-segment
        sums of d(h1_pre)."""
        sh = self.sh
        B, T, M, L = a["B"], a["T"], a["M"], a["L"]
        S, E, H, D, P = sh.S, sh.E, sh.H, sh.D, sh.P
        pe = a["pdrop"][0]
        pre = "decoder.gpt2.transformer."
        nty = min(32, sh.V)
        hip.embed_add_bwd(dx, a["type_ids"], self.G(pre + "wpe.weight"), self.G(pre + "wte.weight"), M, T, D,
                          nty, drop_p=pe, drop_seed=a["seed"],
                          ws=self.buf("embed_bwd_ws", (int(hip.lib().mmtg_embed_add_bwd_ws(M, D, nty)),), torch.float32))
        self._ready("wpe")
        dh1 = self.buf("d_h1", (M, H))
        px3 = bool(a.get("px3"))
        if px3:
            # split-precision projector backward: d h1_pre = (dx W2) (1 - h1^2) through the [in,out] plane copy of W2, and BOTH
            # weight gradients (W2: dx^T h1, W1: d h1_pre^T X) in one grouped launch on plane pairs
            dxp = hip.split_planes(dx, M, D, self.pbuf("d_resid0_p", M, D))
            dh1p = self.pbuf("d_h1_p", M, H)
            hip.gemm_x3(dxp, self.Wtx("decoder.projector_layer2.weight"), dh1, M, H, D, planes=dh1p, epi=hip.EPI_DTANH, aux=a["h1"], ldaux=H)
            # (counters of its own: the blocks' deferred launches may be running on the side stream by now -- _WGRAD_TAIL)
            bufs = self._group_bufs(((D, H), (H, E)), 0, lambda tiles: _group_splits_x3(tiles, M), "wgrad_group_ws_proj", "wgrad_group_cnt_proj")
            pkeys = ("decoder.projector_layer2.weight", "decoder.projector_layer1.weight")
            for k in pkeys:      # (tensors the lazy zero_grad skipped are overwritten below; otherwise accumulate as ever)
                if self._lazy is not None and (self.layout.entries[k][0], self.layout.entries[k][2]) in self._lazy and not self.wgrad_overwrite:
                    self.G(k).zero_()
            self._launch_group([(dxp, a["h1p"], self.G(pkeys[0]), D, H), (dh1p, a["xp"], self.G(pkeys[1]), H, E)], M, bufs, _X3_WG_CFG,
                               ((self.layout.entries[k][0], self.layout.entries[k][2]) for k in pkeys))
            hip.colsum(dx, M, D, self.G("decoder.projector_layer2.bias"))
        else:
            self._dgrad(dx, "decoder.projector_layer2.weight", dh1, M, "linear", epi=hip.EPI_DTANH, aux=a["h1"], ldaux=H)
            self._wgrad(a["h1"], dx, "decoder.projector_layer2.weight", "decoder.projector_layer2.bias", M, "linear")
        # d c[b,k] = (sum over the segment's tokens of d h1_pre) W1   (the add is linear)
        seg = self.buf("d_seg", (B * S, H))
        hip.segment_sum(dh1, seg, B, P, L, S, H, sh.two_sents)
        if a["ids32"] is not None:
            # d W1 = d h1_pre^T X with X = E[id] + c[seg] never materialised: the table rows enter the K-strided operand of
            # the weight-gradient product by index (mmtg_gemm_gather mode 1), the c part is the small product seg^T c
            gw = self.G("decoder.projector_layer1.weight")
            splits = _wgrad_splits(H, E, M, True)
            part = self.buf("wgrad_slabs", (splits * H * E,), torch.float32)
            hip.gemm_gather(1, dh1, self.table, part, H, E, M, a["ids32"], self.table.shape[0], lda=H, ldb=E, ldc=E,
                            epi=hip.EPI_SPLIT, splits=splits)
            hip.slab_sum(part, splits, H * E, gw, H * E, accumulate=not self.wgrad_overwrite)
            hip.gemm(seg, a["c"], gw, H, E, B * S, transA=True, transB=False, lda=H, ldb=E, ldc=E, epi=hip.EPI_ATOMIC, splits=1)
            hip.colsum(dh1, M, H, self.G("decoder.projector_layer1.bias"))
        elif px3:
            hip.colsum(dh1, M, H, self.G("decoder.projector_layer1.bias"))      # (the weight gradient went with W2's above)
        else:
            self._wgrad(a["x"], dh1, "decoder.projector_layer1.weight", "decoder.projector_layer1.bias", M, "linear")
        return seg

    def _launch_tail_jobs(self):
        """The deferred blocks' grouped weight gradients, in block order on ONE side stream (they share a workspace and counters; the
        in-loop launches are complete by now): behind everything enqueued so far, beside what the main stream enqueues next."""
        if not self._tail_jobs:
            return
        side = self._side_stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for probs, m_, gs_, gws_, gcnt_, acc_, cfg_ in self._tail_jobs:
                hip.wgrad_group(probs, m_, gs_, gws_, gcnt_, accumulate=acc_, config=cfg_)
        self._tail_jobs = []
        self._tail_side = side

    def _backward_encoder(self, a, seg, dkl):
        """d c = seg W1 -> beta fuser -> alpha attention + LayerNorm + recurrent channels -> topic channel."""
        sh = self.sh
        B, M = a["B"], a["M"]
        S, E, H, D = sh.S, sh.E, sh.H, sh.D
        lnws = self.buf("ln_bwd_ws", (hip.lib().mmtg_layernorm_bwd_ws(M, max(D, H)),), torch.float32)
        dc = self.buf("d_c", (B * S, E))
        self._dgrad(seg, "decoder.projector_layer1.weight", dc, B * S, "linear")
        # ---- beta fuser
        do = self.buf("d_o", (B * S, H))
        self._dgrad(dc, "mm_atten_layer.out_linear.weight", do, B * S, "linear")
        self._wgrad(a["o"], dc, "mm_atten_layer.out_linear.weight", "mm_atten_layer.out_linear.bias", B * S, "linear")
        dtopic = self.buf("d_topic32", (B, H), torch.float32, zero=True)
        dci = self.buf("d_actx_img", (B * S, H))
        dct = self.buf("d_actx_text", (B * S, H))
        hip.beta_fuse_bwd(a["t_ln"], a["alpha"]["img"][1], a["alpha"]["text"][1], self.Pp("att_w"), a["ba"], do,
                          dtopic, dci, dct, self.Gp("att_w"), self.Gp("att_b"), B, S, H)
        self._ready("att_b")
        # ---- alpha attention + LayerNorm + GRU per modality
        for mod, ch, lnk, dctx_a in (("text", "text", "ln_layer3", dct), ("img", "image", "ln_layer2", dci)):
            dhp32 = self.buf("d_hp32", (B, H), torch.float32)
            tmp32 = self.buf("d_tmp32", (B, H), torch.float32)
            lnws_m = self.buf("ln_bwd_ws", (hip.lib().mmtg_layernorm_bwd_ws(M, max(D, H)),), torch.float32)
            qkv_a, _, probs = a["alpha"][mod]
            layers, h_ln = a["enc"][ch]
            h_all = layers[-1]["h"]
            dqkv_a = self.buf("d_aqkv", (B * S, 3 * H))
            hip.alpha_attn_bwd(qkv_a, self.prior, probs, dctx_a, dkl, dqkv_a, B, S, H, sh.heads)
            dhln = self.buf("d_hln", (B * S, H))
            if not self._gemm_few_rows(dqkv_a, self.Wp(mod + "_qkv_w"), dhln, B * S, H, 3 * H, False, H):
                hip.gemm(dqkv_a, self.Wp(mod + "_qkv_w"), dhln, B * S, H, 3 * H, transB=False, ldb=H)
            hip.gemm(dqkv_a, h_ln, self.Gp(mod + "_qkv_w"), 3 * H, H, B * S, transA=True, transB=False, lda=3 * H,
                     ldb=H, ldc=H, epi=hip.EPI_ATOMIC, splits=1)
            hip.colsum(dqkv_a, B * S, 3 * H, self.Gp(mod + "_qkv_b"))
            dh_all = self.buf("d_hall", (B * S, H))
            hip.layernorm_bwd(dhln, h_all, self.P(lnk + ".weight"), *a["st"][lnk], None, dh_all,
                              self.G(lnk + ".weight"), self.G(lnk + ".bias"), B * S, H, ws=lnws_m)
            self._rnn_bwd(ch, layers, dh_all, B, dhp32, tmp32)
        # ---- topic channel
        dt_ln = self.buf("d_tln", (B, H))
        hip.cast_f32_to(dtopic, dt_ln, B * H)
        dt_raw = self.buf("d_traw", (B, H))
        hip.layernorm_bwd(dt_ln, a["t_raw"], self.P("ln_layer1.weight"), *a["st"]["ln1"], None, dt_raw,
                          self.G("ln_layer1.weight"), self.G("ln_layer1.bias"), B, H, ws=lnws)
        self._wgrad(a["xt"], dt_raw, "encoder.topic_fc.weight", "encoder.topic_fc.bias", B, "linear")
        self._ready("encoder.topic_fc.bias")

    def _rnn_bwd(self, ch, layers, dh_all, B, dhp32, tmp32):
        """BPTT of one encoder channel (rows b*S+t), top layer first.  dh_all [B*S, H]: gradient of the top layer's outputs."""
        sh = self.sh
        S, H = sh.S, sh.H
        kind, NL = sh.rnn[ch]
        G = hip.RNN_GATES[kind]
        r = f"encoder.rnns_{ch}."
        for l in range(NL - 1, -1, -1):
            sfx = "_l%d" % l
            rec = layers[l]
            h_all, save = rec["h"], rec["save"]
            dgi = self.buf("d_gi%d" % G, (B * S, G * H))
            if kind == "GRU":
                # every step's d(gh) is kept (time-major) so that the recurrent weight / bias gradients are ONE
                # product and ONE column sum after the loop instead of one per step
                dgh_tm = self.buf("d_gh_tm", (S, B, 3 * H))
                ks = 6 if (3 * H) % (6 * 64) == 0 else 0      # split-K slabs of the carry product (fp32 kernel too, round 5: 92 -> us per step)
                part = self.buf("d_hp_slabs", (max(ks, 1), B, H), torch.float32)
                for t in range(S - 1, -1, -1):
                    # total gradient wrt h_t = rows b*S+t of dh_all + carry dh_{t+1} z_{t+1} + d(gh_{t+1}) W_hh, assembled in the cell kernel
                    last = t == S - 1
                    dgh = dgh_tm[t]
                    hip.gru_cell_bwd_fused(dh_all[t:], S * H, None if last else dhp32, None if last else (part if ks else tmp32),
                                           0 if last else (ks or 1), save[t], None if t == 0 else h_all[t - 1:], dgi[t:], dgh, dhp32,
                                           B, H, ld_hp=S * H, ld_dgi=S * 3 * H)
                    if t > 0:
                        if ks:
                            hip.gemm(dgh, self.W(r + "weight_hh" + sfx), part, B, H, 3 * H, transB=False, ldb=H,
                                     epi=hip.EPI_SPLIT, out_f32=True, splits=ks)
                        else:
                            hip.gemm(dgh, self.W(r + "weight_hh" + sfx), tmp32, B, H, 3 * H, transB=False, ldb=H, out_f32=True)
                hip.colsum(dgh_tm, S * B, 3 * H, self.G(r + "bias_hh" + sfx))
                drec_tm = dgh_tm[1:]
            else:
                # LSTM / ReLU cell: d(gi) = d(gh) = d(pre-activation), one tensor
                lstm = kind == "LSTM"
                code = hip.RNN_LSTM if lstm else hip.RNN_RELU
                dc = self.buf("d_c32", (B, H), torch.float32) if lstm else None
                for t in range(S - 1, -1, -1):
                    last = t == S - 1
                    hip.rnn_cell_bwd(code, dh_all[t:], S * H, None if last else tmp32, save[t] if lstm else None,
                                     rec["c"][t - 1] if lstm and t else None, h_all[t:], S * H, dc, not last, dgi[t:], S * G * H, B, H)
                    if t > 0:
                        hip.gemm(dgi[t:], self.W(r + "weight_hh" + sfx), tmp32, B, H, G * H, transB=False, lda=S * G * H, ldb=H,
                                 out_f32=True)
                hip.colsum(dgi, B * S, G * H, self.G(r + "bias_hh" + sfx))
                drec_tm = None
                if S > 1:
                    drec_tm = self.buf("d_a_tm%d" % G, (S - 1, B, G * H))
                    drec_tm.copy_(dgi.view(B, S, G * H)[:, 1:].transpose(0, 1))     # data movement only
            if S > 1:
                hprev_tm = self.buf("h_prev_tm", (S - 1, B, H))
                hprev_tm.copy_(h_all.view(B, S, H)[:, :S - 1].transpose(0, 1))     # data movement only
                hip.gemm(drec_tm, hprev_tm, self.G(r + "weight_hh" + sfx), G * H, H, (S - 1) * B, transA=True, transB=False,
                         lda=G * H, ldb=H, ldc=H, epi=hip.EPI_ATOMIC, splits=1)
            self._wgrad(rec["inp"], dgi, r + "weight_ih" + sfx, r + "bias_ih" + sfx, B * S, "linear")
            if l > 0:
                # gradient of the layer below's outputs: d(gi) W_ih, through the same dropout mask as the forward
                dh_all = self.buf("d_hx%d" % (l & 1), (B * S, H))
                hip.gemm(dgi, self.W(r + "weight_ih" + sfx), dh_all, B * S, H, G * H, transB=False, ldb=H)
                if layers[l - 1]["drop"] is not None:
                    hip.dropout_apply(dh_all, dh_all, B * S * H, sh.rnn_pdrop, layers[l - 1]["drop"])

    # ---------------------------------------------------------------- optimizer (train.py:194-197)
    def grad_norm_sq(self):
        hip.sumsq(self.grad, self.layout.total, self.normsq)        # (written, in a fixed order: no memset, no atomics)
        return self.normsq

    def group_norm_sq(self, groups):
        """Per-group sums of squares of the gradient (hip.GroupTable `groups`) into self.group_normsq[:ngroups]; the trainable
        groups' total lands in self.normsq[0], which is the last element of the same buffer: the norm clip_grad_norm_ sees when
        frozen parameters have no gradient."""
        if self.group_normsq is None or self.group_normsq.numel() != groups.ngroups + 1:
            self.group_normsq = torch.zeros(groups.ngroups + 1, device=self.dev)
            self.normsq = self.group_normsq[groups.ngroups:]
        hip.sumsq_groups(self.grad, self.layout.total, groups, self.group_normsq)
        return self.normsq

    def adamw_step(self, lr, max_norm=1.0, betas=(0.9, 0.999), eps=1e-6, wd=0.0, grad_scale=1.0, clip=True, count=None, groups=None):
        """clip_grad_norm_(1.0) + transformers.AdamW(lr, eps=1e-6, wd=0) over the flat buffers,
        refreshing the bf16 weight copies in the same pass.  count: device scalar, the global row count when the
        flat buffer holds row SUMS (mmtg_adamw divides by it; zero rows = no update).
        groups: a hip.GroupTable -- the step then runs per parameter group (lr * lr_scale, the group's weight decay in place of
        `wd`, frozen groups untouched) through mmtg_sumsq_groups + mmtg_adamw_groups; None is the plain step."""
        if self.opt_m is None:
            self.opt_m = torch.zeros_like(self.master)
            self.opt_v = torch.zeros_like(self.master)
        self.step_count += 1
        p_hi = self.wc2[0] if self.x3 else None if self.dtype == hip.F32 else self.wc
        p_lo = self.wc2[1] if self.x3 else None
        if groups is None:
            ns = self.grad_norm_sq() if clip else None
            hip.adamw(self.master, self.grad, self.opt_m, self.opt_v, p_hi,
                      self.layout.total, lr, betas[0], betas[1], eps, wd, self.step_count, ns, max_norm, grad_scale, count=count,
                      p_lo=p_lo)
        else:
            ns = self.group_norm_sq(groups) if clip else None
            hip.adamw_groups(self.master, self.grad, self.opt_m, self.opt_v, p_hi, self.layout.total, groups, lr, betas[0], betas[1],
                             eps, self.step_count, ns, max_norm, grad_scale, count=count, p_lo=p_lo)
        self._refresh_transposed()
        self.copies_fresh = True

    # ---------------------------------------------------------------- weight averaging
    def ema_update(self, w, count=None):
        """ema += w (master - ema) over the whole flat buffer (hip.ema_update), w = 1 - decay.  The first call allocates `ema` as a
        copy of the master -- data movement, no arithmetic -- so a caller that wants the average to start from the weights BEFORE an
        optimizer step makes that call's copy first (MMTGTrainer._close_end does).  Pads, gaps and frozen tensors are equal in both
        buffers and stay so bit for bit.  count: adamw_step's device scalar; a step it skipped skips the average."""
        self.ema_init()
        hip.ema_update(self.ema, self.master, self.layout.total, w, count=count)

    def ema_init(self):
        """Allocate `ema` as a copy of the master if there is none yet."""
        if self.ema is None:
            self.ema = self.master.detach().clone()

    def swap_ema(self):
        """Exchange master and average in place, bit for bit (hip.swap_f32); every derived copy -- the bf16 copy, the (hi | lo)
        planes, the [out,in] transposes, the decoders' folds -- is re-derived by the next forward() or generation through
        refresh_copies().  All pointers stay valid: captured decode graphs replay over the swapped data."""
        if self.ema is None:
            raise RuntimeError("Engine.swap_ema: there is no average yet (ema_update has not run)")
        hip.swap_f32(self.master, self.ema, self.layout.total)
        self.invalidate_copies()
