"""The constraints of a generation, checked and packed on the host before any device work (prefix, n-gram size, beam groups; line
bounds / end sets / templates / rhyme scheme / refrain scheme as LineTables), and the host-side scoring of token log-probabilities.
numpy and Python only: decode.py uploads the tables and chooses the launches, include/mmtg_hip.h states the rules the kernels apply."""
from __future__ import annotations

import math

import numpy as np
import torch

BANNED = (1, 2, 100, 102)           # never a content id: [#START#] [#EOS#] [UNK] [SEP] (src/generate.py:135)


def check_prefix(prefix, rows, length, sent=22, V=None):
    """Validate a prefixed generation's opening lyric ids on the host, before any device work; returns one list of ids per row.

    prefix: a [rows, Lmax] integer tensor / array padded with -1, or a list of `rows` id lists.  Row b's prefix p (L >= 1 ids) is
    lyric columns 0 .. L - 1 in the slot layout of the training data (data.MyDataset): column c holds [#START#] (1) where
    c % sent == 0, [#EOS#] (2) where c % sent == sent - 1, and a content id or PAD (0) elsewhere -- never one of the banned ids
    1, 2, 100, 102.  So p is whole lines (L % sent == 1: it ends on the next line's [#START#]) or whole lines plus a partial line.
    L <= length + 1: the output has 1 + length columns."""
    if isinstance(prefix, (list, tuple)):
        ids = [[int(v) for v in np.asarray(r).reshape(-1).tolist()] for r in prefix]
    else:
        a = prefix.detach().cpu().numpy() if torch.is_tensor(prefix) else np.asarray(prefix)
        if a.ndim != 2:
            raise ValueError("prefix must be a [rows, Lmax] array padded with -1 or a list of id lists (got shape %s)" % (a.shape,))
        ids = []
        for r in a.tolist():
            n = r.index(-1) if -1 in r else len(r)
            if any(v != -1 for v in r[n:]):
                raise ValueError("prefix row %d: ids after the -1 padding" % len(ids))
            ids.append([int(v) for v in r[:n]])
    if len(ids) != rows:
        raise ValueError("prefix has %d rows, the generation %d" % (len(ids), rows))
    for b, p in enumerate(ids):
        if not p:
            raise ValueError("prefix row %d is empty (it starts with [#START#])" % b)
        if len(p) > length + 1:
            raise ValueError("prefix row %d has %d ids, more than length + 1 = %d" % (b, len(p), length + 1))
        for c, v in enumerate(p):
            if c % sent == 0 and v != 1:
                raise ValueError("prefix row %d, column %d: [#START#] (1) expected, got %d" % (b, c, v))
            if c % sent == sent - 1 and v != 2:
                raise ValueError("prefix row %d, column %d: [#EOS#] (2) expected, got %d" % (b, c, v))
            if 0 < c % sent < sent - 1 and (v in BANNED or v < 0 or (V is not None and v >= V)):
                raise ValueError("prefix row %d, column %d: id %d is not a content id or PAD" % (b, c, v))
    return ids


def check_ngram(n, sent=22):
    """Validate no_repeat_ngram_size on the host, before any device work; returns it as an int.  0 is off; 1 .. sent - 2 blocks
    every content n-gram a row already holds (include/mmtg_hip.h states the rule; a longer n-gram can never be all content).
    Bools and non-integers raise ValueError, as do values out of range."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise ValueError("no_repeat_ngram_size must be an integer, got %r" % (n,))
    n = int(n)
    if not 0 <= n <= sent - 2:
        raise ValueError("no_repeat_ngram_size %d outside 0..%d (sent - 2)" % (n, sent - 2))
    return n


def check_groups(num_beams, num_beam_groups=1, diversity_penalty=0.0):
    """The beam groups of a diverse beam search: (G, penalty) for `num_beams` beams.  1 <= G <= num_beams and G divides num_beams;
    the penalty is finite and >= 0, and 0 unless G > 1 (a penalty on one group would do nothing: that is a mistake, not a setting)."""
    nb = int(num_beams)
    if not _is_int(num_beam_groups):
        raise ValueError("num_beam_groups must be an integer, got %r" % (num_beam_groups,))
    G = int(num_beam_groups)
    if not 1 <= G <= nb or nb % G:
        raise ValueError("num_beam_groups %d must be in 1..%d and divide num_beams %d" % (G, nb, nb))
    lam = float(diversity_penalty)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("diversity_penalty must be finite and >= 0, got %r" % (diversity_penalty,))
    if G == 1 and lam != 0.0:
        raise ValueError("diversity_penalty %r needs num_beam_groups > 1 (one group has no earlier group to differ from)" % (diversity_penalty,))
    return G, lam


def check_contrastive(top_k, penalty_alpha):
    """The settings of a contrastive search: (k, alpha).  k candidates per step, an integer in 1..16 (a prompt's rows, the beam
    decoder's layout); alpha in [0, 1] weighs the degeneration penalty against the model's probability (0: greedy decoding)."""
    if not _is_int(top_k):
        raise ValueError("top_k must be an integer, got %r" % (top_k,))
    k = int(top_k)
    if not 1 <= k <= 16:
        raise ValueError("top_k %d outside 1..16" % k)
    try:
        alpha = float(penalty_alpha)
    except (TypeError, ValueError):
        raise ValueError("penalty_alpha must be a number, got %r" % (penalty_alpha,)) from None
    if not 0.0 <= alpha <= 1.0:                  # (NaN fails both comparisons)
        raise ValueError("penalty_alpha must be in [0, 1], got %r" % (penalty_alpha,))
    return k, alpha


WARP_OFF = (0.0, 1.0, 0.0, 0.0)        # (min_p, typical_p, epsilon_cutoff, eta_cutoff) at which every stage is off


def check_warp(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """The four truncation settings of a sampled generation beyond top_k / top_p, with the names, defaults and ranges of
    transformers' generate: (min_p, typical_p, epsilon_cutoff, eta_cutoff) as floats.  min_p in [0, 1] (0 off), typical_p in (0, 1]
    (1 off), epsilon_cutoff and eta_cutoff in [0, 1) (0 off); anything else (a NaN, a non-number) raises a ValueError that names the
    argument.  include/mmtg_hip.h states the rule, ``warp_filter`` restates it."""
    out = []
    for name, v, ok, rng in (("min_p", min_p, lambda a: 0.0 <= a <= 1.0, "[0, 1]"),
                             ("typical_p", typical_p, lambda a: 0.0 < a <= 1.0, "(0, 1]"),
                             ("epsilon_cutoff", epsilon_cutoff, lambda a: 0.0 <= a < 1.0, "[0, 1)"),
                             ("eta_cutoff", eta_cutoff, lambda a: 0.0 <= a < 1.0, "[0, 1)")):
        try:
            if isinstance(v, (bool, np.bool_, str, bytes)):
                raise TypeError
            a = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number in %s, got %r" % (name, rng, v)) from None
        if not ok(a):                            # (NaN fails every comparison)
            raise ValueError("%s must be in %s, got %r" % (name, rng, v))
        out.append(a)
    return tuple(out)


def _warp_row(x, min_p, typical_p, epsilon_cutoff, eta_cutoff, margins):
    keep = x > -np.inf

    def softmax():
        """p, log p and the entropy over the survivors (a dropped id has p = 0; 0 log 0 = 0), and who holds their maximum"""
        m = x[keep].max()
        e = np.where(keep, np.exp(np.where(keep, x - m, 0.0)), 0.0)
        tot = e.sum()
        logp = np.where(keep, (x - m) - np.log(tot), -np.inf)
        p = e / tot
        pos = p > 0.0
        return p, logp, -(p[pos] * logp[pos]).sum(), keep & (x == m)

    def cut_probabilities(thr, what):
        nonlocal keep
        p, _, _, top = softmax()
        if margins is not None and thr > 0.0:
            margins.append((what, "probability", float(np.abs(p[keep] - thr).min() / thr)))
        keep = keep & ((p >= thr) | top)

    if min_p > 0.0:
        cut_probabilities(min_p * softmax()[0].max(), "min_p")
    if typical_p < 1.0:
        p, logp, H, _ = softmax()
        key = np.where(p > 0.0, np.abs(-logp - H), np.inf)
        order = np.flatnonzero(keep)
        order = order[np.argsort(key[order], kind="stable")]
        cum = np.cumsum(p[order])
        reached = np.flatnonzero(cum >= typical_p)
        if margins is not None:
            ends = np.append(key[order][1:] != key[order][:-1], True)          # the mass as the ids of one key arrive together
            margins.append(("typical_p", "mass", float(np.abs(cum[ends] - typical_p).min())))
        if reached.size:
            cut = key[order[reached[0]]]
            if margins is not None:
                away = np.abs(key[order] - cut)[key[order] != cut]
                margins.append(("typical_p", "key", float(away.min()) if away.size else np.inf))
            keep = keep & (key <= cut)
    if epsilon_cutoff > 0.0:
        cut_probabilities(epsilon_cutoff, "epsilon_cutoff")
    if eta_cutoff > 0.0:
        H = softmax()[2]
        cut_probabilities(min(eta_cutoff, math.sqrt(eta_cutoff) * math.exp(-H)), "eta_cutoff")
    return np.where(keep, x, -np.inf)


def warp_filter(logits, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, margins=None):
    """The four truncation stages of the *_warp entries (include/mmtg_hip.h) in float64 numpy, the host's statement of the rule and the
    tests' oracle: transformers' MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper with
    min_tokens_to_keep = 1, chained in that order.  logits [V] or [rows, V]: the processed logits after the top-k / top-p filters
    (-inf where dropped or banned).  Returns a float64 array of the same shape, -inf where a stage dropped the id.  Each stage sees the
    softmax over the survivors of the stages before it.  margins (a list, optional) receives (argument, kind, distance) per row and
    active stage -- how far the nearest id lies from the stage's cut: "probability" relative to the cut, the typical stage's "key"
    absolute (ids at the cut key itself aside) and its accumulated "mass" absolute -- for tests that compare an fp32 evaluation."""
    warp = check_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    x = np.asarray(logits, dtype=np.float64)
    rows = x.reshape(-1, x.shape[-1])
    out = np.stack([r.copy() if not (r > -np.inf).any() else _warp_row(r, *warp, margins) for r in rows])
    return out.reshape(x.shape)


MIROSTAT_OFF = (0.0, 0.1)              # (mirostat_tau, mirostat_eta): tau = 0 is off, eta is llama.cpp's default


def check_mirostat(mirostat_tau=0.0, mirostat_eta=0.1):
    """The two Mirostat settings of a sampled generation, with llama.cpp's names: (mirostat_tau, mirostat_eta) as floats.  mirostat_tau
    is 0 (off) or in (0, 32], mirostat_eta in [0, 1]; anything else (a NaN, a non-number) raises a ValueError that names the argument.
    include/mmtg_hip.h states the rule, ``mirostat_filter`` and ``mirostat_update`` restate it."""
    out = []
    for name, v, ok, rng in (("mirostat_tau", mirostat_tau, lambda a: 0.0 <= a <= 32.0, "0 (off) or (0, 32]"),
                             ("mirostat_eta", mirostat_eta, lambda a: 0.0 <= a <= 1.0, "[0, 1]")):
        try:
            if isinstance(v, (bool, np.bool_, str, bytes)):
                raise TypeError
            a = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, %s, got %r" % (name, rng, v)) from None
        if not ok(a):                            # (NaN fails every comparison)
            raise ValueError("%s must be %s, got %r" % (name, rng, v))
        out.append(a)
    return tuple(out)


def mirostat_filter(x, mu, margins=None):
    """The Mirostat v2 cut of the *_mirostat entries (include/mmtg_hip.h) in float64 numpy: x [V] is a row of processed logits after
    every earlier stage (``warp_filter``'s result; -inf where dropped), mu the row's state in bits.  With p the softmax over the
    survivors, an id stays when -log2 p <= mu or when it holds the survivors' largest logit.  Returns the filtered row.  margins (a
    list, optional) receives ("mirostat_tau", "surprise", |-log2 p - mu|) for every survivor, in index order -- how far each lies
    from the cut, in bits, for tests that compare an fp32 evaluation."""
    x = np.asarray(x, dtype=np.float64)
    keep = x > -np.inf
    if not keep.any():
        return x.copy()
    m = x[keep].max()
    surprise = -((x[keep] - m) - np.log(np.exp(x[keep] - m).sum())) / math.log(2.0)
    if margins is not None:
        margins.extend(("mirostat_tau", "surprise", float(d)) for d in np.abs(surprise - float(mu)))
    out = np.full_like(x, -np.inf)
    stay = np.flatnonzero(keep)[(surprise <= float(mu)) | (x[keep] == m)]
    out[stay] = x[stay]
    return out


def mirostat_update(filtered, pick, mu, tau, eta):
    """What drawing id `pick` from the row ``mirostat_filter`` returned does to the state: (s, mu') with s = -log2 q(pick) under the
    softmax q over the kept ids and mu' = mu - eta * (s - tau), in float64."""
    f = np.asarray(filtered, dtype=np.float64)
    keep = f > -np.inf
    if not keep[pick]:
        raise ValueError("mirostat_update: id %d is not in the kept set" % pick)
    m = f[keep].max()
    s = (math.log(np.exp(f[keep] - m).sum()) - (f[pick] - m)) / math.log(2.0)
    return float(s), float(mu) - float(eta) * (float(s) - float(tau))


def check_stochastic(num_samples, seed=0):
    """The settings of a stochastic beam search: (nb, seed).  nb samples without replacement per prompt, an integer in 1..16 (a
    prompt's rows, the beam decoder's layout); seed an integer in 0 .. 2^32 - 1, the word every row's noise is derived from
    (``stochastic_row_seeds``).  Anything else raises a ValueError that names the argument."""
    if not _is_int(num_samples):
        raise ValueError("num_samples must be an integer, got %r" % (num_samples,))
    nb = int(num_samples)
    if not 1 <= nb <= 16:
        raise ValueError("num_samples %d outside 1..16" % nb)
    if not _is_int(seed):
        raise ValueError("seed must be an integer, got %r" % (seed,))
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("seed %d outside 0 .. 2^32 - 1" % int(seed))
    return nb, int(seed)


def _hash_u32(seed, idx):
    """hash_u32 of csrc/common.h (the murmur3 finaliser over seed + idx * 0x9E3779B1) on numpy uint32 arrays, bit-exact."""
    with np.errstate(over="ignore"):
        h = np.asarray(idx, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.asarray(seed, dtype=np.uint32)
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        return h ^ (h >> np.uint32(16))


def stochastic_row_seeds(seed, first_prompt, n_prompts, nb):
    """The row_seed words of mmtg_decode_gumbel_candidates for prompts first_prompt .. first_prompt + n_prompts - 1 of a call, uint32
    [n_prompts * nb] in the decoder's row order: hash(hash(seed, 1 + the prompt's index in the whole call), 1 + the beam slot) (from
    1: the hash maps (0, 0) to 0).  The batch chunk is not an input, so how a call is cut into batches does not change a prompt's
    noise."""
    nb, seed = check_stochastic(nb, seed)
    prompts = np.arange(int(first_prompt), int(first_prompt) + int(n_prompts), dtype=np.uint64) + np.uint64(1)
    return _hash_u32(_hash_u32(np.uint32(seed), prompts.astype(np.uint32))[:, None],
                     np.arange(1, nb + 1, dtype=np.uint32)[None, :]).reshape(-1)


def gumbel_uniforms(seed_words, pos, V):
    """u of the noise rule (include/mmtg_hip.h) as float32 [rows, V], the kernel's bits: h = hash(hash(row_seed[b], pos), v),
    u = ((h >> 9) + 0.5) * 2^-23 -- exact in fp32 and strictly inside (0, 1)."""
    words = np.asarray(seed_words, dtype=np.uint32).reshape(-1)
    h = _hash_u32(_hash_u32(words, np.uint32(int(pos) & 0xFFFFFFFF))[:, None], np.arange(int(V), dtype=np.uint32)[None, :])
    return ((h >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def gumbel_noise(seed_words, pos, V):
    """n_v = -log(-log(u)) of the noise rule in float64 [rows, V], from the exact u of ``gumbel_uniforms``: nothing random is left."""
    return -np.log(-np.log(gumbel_uniforms(seed_words, pos, V).astype(np.float64)))


def _log1mexp(a):
    """log(1 - exp(a)) for a <= 0 in float64; log1mexp(0) = -inf."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(a > -math.log(2.0), np.log(-np.expm1(a)), np.log1p(-np.exp(np.minimum(a, 0.0))))


def gumbel_candidates(x, scores, gum, seed_words, pos, nb, only=None, gaps=None):
    """mmtg_decode_gumbel_candidates (include/mmtg_hip.h) in float64 numpy, the host's statement of the rule and the tests' oracle.
    x [rows, V]: the processed logits of every row (penalty, temperature and every ban applied; -inf where banned); scores / gum
    [rows]; seed_words uint32 [rows]; pos the step's position.  only (optional) [rows]: the id of a row that sits on a single-choice
    column (a copy, a sticky or full-line PAD, a given id), -1 elsewhere.  Returns (cand_id int64, cand_val, cand_g float64), each
    [rows, nb]: per row the nb largest t = log_softmax(x) + noise by (t descending, id ascending), their log-probabilities and the
    children's perturbed values; a dead row (gum or score not above -inf) and a row with every id banned offer -inf and id 0.
    gaps (a list, optional) receives per row the gap between its nb-th and (nb + 1)-th t (inf where nothing was to decide)."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    R, V = x.shape
    scores, gum = np.asarray(scores, dtype=np.float64).reshape(R), np.asarray(gum, dtype=np.float64).reshape(R)
    noise = gumbel_noise(seed_words, pos, V)
    ids = np.zeros((R, nb), dtype=np.int64)
    val, g = np.full((R, nb), -np.inf), np.full((R, nb), -np.inf)
    for b in range(R):
        gap = np.inf
        live = gum[b] > -np.inf and scores[b] > -np.inf
        if live and only is not None and only[b] >= 0:
            ids[b, 0], val[b, 0], g[b, 0] = int(only[b]), 0.0, gum[b]
        elif live and (x[b] > -np.inf).any():
            ok = x[b] > -np.inf
            m = x[b][ok].max()
            lp = np.where(ok, (x[b] - m) - math.log(np.exp(x[b][ok] - m).sum()), -np.inf)
            t = np.where(ok, lp + noise[b], -np.inf)
            order = np.lexsort((np.arange(V), -t))
            zt = t[order[0]]
            for r, v in enumerate(order[:nb]):
                if not ok[v]:
                    break
                w = (gum[b] - (scores[b] + t[v])) + float(_log1mexp(t[v] - zt))
                ids[b, r], val[b, r] = v, lp[v]
                g[b, r] = gum[b] - max(0.0, w) - math.log1p(math.exp(-abs(w)))
            if V > nb and ok[order[nb - 1]]:
                gap = t[order[nb - 1]] - t[order[nb]]
        if gaps is not None:
            gaps.append(float(gap))
    return ids, val, g


def gumbel_merge(cand_val, cand_id, cand_g, scores, gum, seq, keep, rows, pos, P, sent, nb, fixed_end=None, gaps=None):
    """mmtg_decode_gumbel_merge (include/mmtg_hip.h) on numpy arrays, in place: cand_val / cand_id / cand_g [B, nb] (all None: a step
    without candidates), scores / gum [B], seq / keep / rows [B, width], B a multiple of nb.  Per prompt the nb candidates with the
    largest cand_g by (cand_g descending, parent ascending, rank ascending; a NaN counts as -inf) become its rows in that order:
    columns 0 .. pos of seq / keep / rows are the parent's, seq[b, pos + 1] the id, rows[b, pos + 1] = b, scores[b] = scores[parent] +
    cand_val (a NaN counts as -inf), gum[b] = cand_g.  A held prompt, a forced cadence column and a step without candidates keep
    every row (and gum) and append the forced token, if any.  gaps (a list, optional) receives per merged prompt the gap between
    its nb-th and (nb + 1)-th cand_g (inf where there is no (nb + 1)-th or the nb-th is -inf).  Returns the parents int64 [B] (the
    identity where nothing was merged)."""
    B = scores.shape[0]
    j = pos + 1 - P
    forced = j > 1 and ((j + 1) % sent == 0 or (j + 1) % sent == 1)
    par = np.arange(B, dtype=np.int64)
    for b0 in range(0, B, nb):
        blk = slice(b0, b0 + nb)
        if fixed_end is not None and pos + 1 < fixed_end[b0]:
            rows[blk, pos + 1] = np.arange(b0, b0 + nb)
            continue
        if j < 1 or forced or cand_val is None:
            if j >= 1 and forced:
                seq[blk, pos + 1] = 2 if (j + 1) % sent == 0 else 1
            rows[blk, pos + 1] = np.arange(b0, b0 + nb)
            continue
        cg = np.asarray(cand_g[blk], dtype=np.float64).reshape(-1).copy()
        cg[np.isnan(cg)] = -np.inf
        order = np.lexsort((np.arange(nb * nb), -cg))[:nb]
        if gaps is not None:
            rest = np.lexsort((np.arange(nb * nb), -cg))
            gaps.append(float(cg[rest[nb - 1]] - cg[rest[nb]]) if nb * nb > nb and cg[rest[nb - 1]] > -np.inf else float("inf"))
        p, k = order // nb, order % nb
        with np.errstate(invalid="ignore"):
            sc = (scores[blk][p] + cand_val[blk][p, k]).astype(scores.dtype)
        sc[np.isnan(sc)] = -np.inf
        for t in (seq, keep, rows):
            t[blk, :pos + 1] = t[blk, :pos + 1][p]
        seq[blk, pos + 1] = cand_id[blk][p, k]
        rows[blk, pos + 1] = np.arange(b0, b0 + nb)
        scores[blk] = sc
        gum[blk] = cg[order].astype(gum.dtype)
        par[blk] = b0 + p
    return par


GUIDANCE_OFF = 1.0                     # guidance_scale at which the surface runs the plain decoder


def check_guidance(guidance_scale=GUIDANCE_OFF):
    """The scale of classifier-free guidance, transformers' argument of that name, as a float: a finite real number >= 0 (0 follows the
    negative prompt alone, 1 the prompt alone, more sharpens the prompt against the negative).  Anything else (a bool, a string, None,
    NaN, inf, a negative) raises a ValueError that names the argument.  include/mmtg_hip.h states the rule, ``guidance_scores``
    restates it."""
    try:
        if isinstance(guidance_scale, (bool, np.bool_, str, bytes)):
            raise TypeError
        a = float(guidance_scale)
    except (TypeError, ValueError):
        raise ValueError("guidance_scale must be a number, finite and >= 0, got %r" % (guidance_scale,)) from None
    if not (0.0 <= a < math.inf):               # (NaN fails every comparison)
        raise ValueError("guidance_scale must be finite and >= 0, got %r" % (guidance_scale,))
    return a


def _log_softmax64(x):
    """Row-wise log-softmax in float64; a row without a finite entry comes back all -inf."""
    m = x.max(axis=-1, keepdims=True)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = safe + np.log(np.exp(x - safe).sum(axis=-1, keepdims=True))
        return np.where(np.isfinite(m), x - lse, -np.inf)


def guidance_scores(cond, uncond, scale):
    """The rule of mmtg_decode_guidance (include/mmtg_hip.h) in float64 numpy: cond / uncond [..., V] are the raw logits of the prompts
    and of their negatives, already cut to the columns the selection reads.  Returns lu + scale * (lc - lu) with lc / lu their
    log-softmax over the last axis; an id where either is -inf gets -inf (never NaN), and so does every id of a pair one of whose rows
    is all -inf."""
    c, u = np.asarray(cond, dtype=np.float64), np.asarray(uncond, dtype=np.float64)
    if c.shape != u.shape:
        raise ValueError("guidance_scores: cond %r and uncond %r differ in shape" % (c.shape, u.shape))
    s = check_guidance(scale)
    lc, lu = _log_softmax64(c), _log_softmax64(u)
    out_ = np.isneginf(lc) | np.isneginf(lu)
    with np.errstate(invalid="ignore"):
        g = lu + s * (lc - lu)
    return np.where(out_, -np.inf, g)


GUIDANCE_BRANCHES = ("u", "i", "t")     # the fixed branch order: without the experience, without the images, without the texts


def check_modality_guidance(guidance_scale=GUIDANCE_OFF, image_guidance_scale=GUIDANCE_OFF, text_guidance_scale=GUIDANCE_OFF):
    """The three scales of per-modality guidance, each as ``check_guidance`` takes it (a ValueError names the argument).  Returns
    (branches, scales): the running branches -- those whose scale differs from 1 -- as a tuple of "u" / "i" / "t" in that order, and
    their scales, a tuple of floats.  A prompt then runs beside len(branches) negatives; () is the unguided call.  The weight the rule
    puts on the prompt's own distribution, 1 + sum(s - 1), may come out negative (three scales at 0 give -2): that is allowed."""
    branches, scales = [], []
    for name, arg, value in (("u", "guidance_scale", guidance_scale), ("i", "image_guidance_scale", image_guidance_scale),
                             ("t", "text_guidance_scale", text_guidance_scale)):
        try:
            s = check_guidance(value)
        except ValueError as e:
            raise ValueError(str(e).replace("guidance_scale", arg, 1)) from None
        if s != GUIDANCE_OFF:
            branches.append(name)
            scales.append(s)
    return tuple(branches), tuple(scales)


def modality_guidance_scores(branches, scales):
    """The rule of mmtg_decode_guidance_multi (include/mmtg_hip.h) in float64 numpy.  branches: [K, ..., V] (or a sequence of K
    arrays), the raw logits of the prompts (branches[0]) and of their K - 1 running negatives in branch order, already cut to the
    columns the selection reads; scales: the K - 1 scales.  Returns g = lc;  g = g + (s_k - 1) * (lc - l_k) for k = 1 .. K - 1 in turn,
    with lc / l_k the log-softmax over the last axis: every scale at 1 (or K = 1) gives lc, one branch is ``guidance_scores``'s
    lu + s (lc - lu) up to rounding, a branch equal to the prompt vanishes exactly.  An id that is -inf in any branch gets -inf (never
    NaN), and so does every id of a prompt one of whose K rows is all -inf."""
    x = [np.asarray(b, dtype=np.float64) for b in branches]
    if len(x) != len(scales) + 1:
        raise ValueError("modality_guidance_scores: %d branches take %d scales, got %d" % (len(x), len(x) - 1, len(scales)))
    if any(b.shape != x[0].shape for b in x):
        raise ValueError("modality_guidance_scores: the branches differ in shape: %r" % ([b.shape for b in x],))
    s = [check_guidance(v) for v in scales]
    ls = [_log_softmax64(b) for b in x]
    dead = np.zeros(x[0].shape, bool)
    for l in ls:
        dead |= np.isneginf(l)
    g = ls[0].copy()
    with np.errstate(invalid="ignore"):
        for l, sk in zip(ls[1:], s):
            g = g + (sk - 1.0) * (ls[0] - l)
    return np.where(dead, -np.inf, g)


def chosen_mask(ids, sent=22, prefix_lens=None):
    """Which columns of generated lyric ids count towards a row's score: bool [B, 1 + length], host only.  Column j >= 1 of row b
    counts iff it is not a cadence column (j % sent not in {0, sent - 1}: the forced [#START#] / [#EOS#]), it lies past the row's
    prefix (j >= prefix_lens[b]; None: no prefix) and the previous column is not PAD (ids[b][j - 1] != 0) -- so the first PAD of a
    line counts (the model ended the line there; in an empty line that is its first content column) and the sticky PADs behind
    it, which no model call decided, do not.
    Columns that a constraint decided (a template's given id, a full line's PAD, a refrain's copied id) count: their value is the
    model's log-probability of that id -- the log-probability node scores whatever the column holds.  Samples of one prompt share
    their constraints, so ranking among them is fair."""
    a = np.asarray(ids.detach().cpu().numpy() if torch.is_tensor(ids) else ids)
    if a.ndim != 2:
        raise ValueError("ids must be [rows, 1 + length] (got shape %s)" % (a.shape,))
    B, n = a.shape
    pl = np.zeros(B, np.int64) if prefix_lens is None else np.asarray(prefix_lens, np.int64).reshape(-1)
    if pl.shape[0] != B:
        raise ValueError("prefix_lens has %d rows, ids %d" % (pl.shape[0], B))
    j = np.arange(n)
    mask = np.zeros((B, n), bool)
    mask[:, 1:] = a[:, :-1] != 0
    mask &= ((j >= 1) & (j % sent != 0) & (j % sent != sent - 1))[None, :]
    mask &= j[None, :] >= pl[:, None]
    return mask


def sequence_scores(ids, logprobs, sent=22, prefix_lens=None, upto=None):
    """(sum float64 [B], count int64 [B]) of the token log-probabilities over chosen_mask's columns below `upto` (None: all; for
    the text generate_samples returns, 1 + the last iteration that called the model: GreedyDecoder.reference_return).  Host only."""
    mask = chosen_mask(ids, sent=sent, prefix_lens=prefix_lens)
    lp = np.asarray(logprobs.detach().cpu().numpy() if torch.is_tensor(logprobs) else logprobs, np.float64)
    if lp.shape != mask.shape:
        raise ValueError("logprobs of shape %s for ids of shape %s" % (lp.shape, mask.shape))
    if upto is not None:
        mask[:, max(int(upto), 0):] = False
    return np.where(mask, lp, 0.0).sum(1), mask.sum(1).astype(np.int64)


class LineTables:
    """The packed line constraints check_lines returns: lo, hi uint8 [rows, n_lines]; set_of int16 [rows, n_lines] (-1: no end set)
    and sets uint32 [n_sets, ceil(V / 32)] (bit v & 31 of word v >> 5: id v is a member), or both None when no line has a set.
    tmpl (templates= only, else None): int32 [rows, n_lines, sent - 2], one symbol per content column -- v >= 0 a given id, -1 free,
    v <= -2 the class `sets[-2 - v]` (classes and end sets share the table); a template's length is folded into lo / hi.
    class_of, lead, distinct (rhyme_scheme= only, else None, None, False): class_of int16 [V], the row of `sets` that is id v's rhyme
    class or -1; lead int8 [rows, n_lines], the leader's line of a follower line or -1; a leader's static end set (the union of the
    classes) is folded into set_of.
    src (refrain_scheme= only, else None): int8 [rows, n_lines], the source's line of a copy line or -1 (check_refrain).  bare: the
    tables were made for src alone -- no line argument was given, lo / hi are the unconstrained (0, sent - 2) -- so the decoders
    upload no line tables for them."""

    def __init__(self, lo, hi, set_of, sets, sent, V, tmpl=None, class_of=None, lead=None, distinct=False, src=None, bare=False):
        self.lo, self.hi, self.set_of, self.sets, self.sent, self.V, self.tmpl = lo, hi, set_of, sets, sent, V, tmpl
        self.class_of, self.lead, self.distinct = class_of, lead, bool(distinct)
        self.src, self.bare = src, bool(bare)

    @property
    def rows(self):
        return self.lo.shape[0]

    def repeat(self, k):
        """Every row k times in place of itself (the beams of a prompt share its constraints)."""
        rep = lambda a: None if a is None else np.repeat(a, k, axis=0)      # noqa: E731
        return LineTables(rep(self.lo), rep(self.hi), rep(self.set_of), self.sets, self.sent, self.V, rep(self.tmpl),
                          self.class_of, rep(self.lead), self.distinct, rep(self.src), self.bare)

    def take(self, idx):
        """Rows idx (a list of row indices) as tables of their own; the sets are shared."""
        sub = lambda a: None if a is None else np.ascontiguousarray(a[idx])      # noqa: E731
        return LineTables(sub(self.lo), sub(self.hi), sub(self.set_of), self.sets, self.sent, self.V, sub(self.tmpl),
                          self.class_of, sub(self.lead), self.distinct, sub(self.src), self.bare)

    def source(self, b, l):
        """The line whose text row b's line l repeats (l is a copy line), or None."""
        if self.src is None or l >= self.src.shape[1] or self.src[b, l] < 0:
            return None
        return int(self.src[b, l])

    def leader(self, b, l):
        """The line whose ending decides the rhyme of row b's line l (l is a follower), or None."""
        if self.lead is None or l >= self.lead.shape[1] or self.lead[b, l] < 0:
            return None
        return int(self.lead[b, l])

    def rhyme_class(self, v):
        """The rhyme class of id v as a frozenset, or None (no scheme, or v has no rhyme)."""
        if self.class_of is None or not 0 <= v < len(self.class_of) or self.class_of[v] < 0:
            return None
        return self.members(int(self.class_of[v]))

    def symbol(self, b, l, c):
        """What row b's template says of content column c of line l: an int (a given id), a frozenset (a class) or None (free, no
        template, or a column / line past it)."""
        if self.tmpl is None or l >= self.tmpl.shape[1] or not 0 <= c < self.tmpl.shape[2]:
            return None
        v = int(self.tmpl[b, l, c])
        return v if v >= 0 else None if v == -1 else self.members(-2 - v)

    def bounds(self, b, l):
        """(lo, hi, end set as a frozenset or None) of row b's line l; a line past the table is unconstrained."""
        if l >= self.lo.shape[1]:
            return 0, self.sent - 2, None
        s = -1 if self.set_of is None else int(self.set_of[b, l])
        return int(self.lo[b, l]), int(self.hi[b, l]), self.members(s) if s >= 0 else None

    def members(self, s):
        """Set s of the table as a frozenset of ids."""
        cache = self.__dict__.setdefault("_members", {})
        if s not in cache:
            w = self.sets[s]
            cache[s] = frozenset(v for v in range(32 * len(w)) if (int(w[v >> 5]) >> (v & 31)) & 1)
        return cache[s]


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_ids(e):
    return isinstance(e, (set, frozenset)) or (isinstance(e, (list, tuple, np.ndarray)) and all(_is_int(v) for v in e))


def _per_row(spec, rows, what, whole, per_row_form):
    """spec as one list of per-line entries per row (or the marker ("all", entry): that entry on every line).  spec is None (no
    entries), one entry for every line (`whole(spec)`), one list for all rows, or one list, entry or None per row
    (`per_row_form(spec)`)."""
    if spec is None:
        return [[] for _ in range(rows)]
    if whole(spec):
        return [("all", spec)] * rows
    if not isinstance(spec, (list, tuple)):
        raise ValueError("%s: a list of per-line entries (or one list per row) expected, got %r" % (what, spec))
    if per_row_form(spec):
        if len(spec) != rows:
            raise ValueError("%s has %d rows, the generation %d" % (what, len(spec), rows))
        out = []
        for r in spec:
            if r is not None and not whole(r) and not isinstance(r, (list, tuple)):
                raise ValueError("%s: a row is None, one entry or a list of per-line entries, got %r" % (what, r))
            out.append([] if r is None else ("all", r) if whole(r) else list(r))
        return out
    return [list(spec)] * rows


def _template_rows(spec, rows):
    """templates as one list of per-line entries per row: one list for all rows, or (a list among the entries marks it) one list or
    None per row."""
    if spec is None:
        return [[] for _ in range(rows)]
    if not isinstance(spec, list):
        raise ValueError("templates: a list of per-line templates (or one such list per row) expected, got %r" % (spec,))
    if any(isinstance(e, list) for e in spec):
        if len(spec) != rows:
            raise ValueError("templates has %d rows, the generation %d" % (len(spec), rows))
        for b, r in enumerate(spec):
            if r is not None and not isinstance(r, list):
                raise ValueError("templates row %d: a list of per-line templates or None expected, got %r" % (b, r))
        return [[] if r is None else r for r in spec]
    return [spec] * rows


def _content_id(v, V):
    return not (v == 0 or v in BANNED or v < 0 or (V is not None and v >= V))


def _id_set(e, V, at, noun, expected="a collection of ids", also=None):
    """The collection of ids e as a frozenset: non-empty, every member a content id below the cut V.  `at` opens every message and
    `noun` names the set in them; also(v), if given, is one more check per id, run in ascending order behind the id's own."""
    if not _is_ids(e) or (isinstance(e, np.ndarray) and e.ndim != 1) or not all(_is_int(v) for v in e):
        raise ValueError("%s: %s expected, got %r" % (at, expected, e))
    ids = frozenset(int(v) for v in e)
    if not ids:
        raise ValueError("%s: the %s is empty" % (at, noun))
    for v in sorted(ids):
        if not _content_id(v, V):
            raise ValueError("%s: id %d is not a content id below the vocabulary cut" % (at, v))
        if also is not None:
            also(v)
    return ids


def _scheme_rows(spec, rows):
    """rhyme_scheme as one string (or None) per row: one string for all rows, or a list with one string or None per row."""
    if isinstance(spec, str):
        spec = [spec] * rows
    elif not isinstance(spec, (list, tuple)) or not all(r is None or isinstance(r, str) for r in spec):
        raise ValueError("rhyme_scheme: a string (or a list with one string or None per row) expected, got %r" % (spec,))
    if len(spec) != rows:
        raise ValueError("rhyme_scheme has %d rows, the generation %d" % (len(spec), rows))
    return ["" if r is None else r for r in spec]


def _rhyme_classes(classes, V):
    """rhyme_classes as a list of frozensets: pairwise disjoint, non-empty sets of content ids below V."""
    if not isinstance(classes, (list, tuple)) or not classes:
        raise ValueError("rhyme_classes: a non-empty list of id sets expected, got %r" % (classes,))
    out, owner = [], {}
    for i, e in enumerate(classes):
        def own(v):
            if v in owner:
                raise ValueError("rhyme_classes: id %d is in classes %d and %d (the classes are disjoint)" % (v, owner[v], i))
            owner[v] = i
        out.append(_id_set(e, V, "rhyme_classes, class %d" % i, "class", also=own))
    return out


class _Draft:
    """The tables of check_lines while its steps fill them, row by row: the arrays of LineTables, the id sets in the order they
    were first seen (`table`; LineTables.sets is packed from it) and, with a scheme, the rhyme classes, their union and `place`."""

    def __init__(self, rows, length, sent, V, templates):
        self.length, self.sent, self.V = length, sent, V
        self.n_lines, self.cap = n_lines, cap = (length - 1) // sent + 1, sent - 2
        self.lo = np.zeros((rows, n_lines), np.uint8)
        self.hi = np.full((rows, n_lines), cap, np.uint8)
        self.set_of = np.full((rows, n_lines), -1, np.int16)
        self.tmpl = np.full((rows, n_lines, cap), -1, np.int32) if templates else None
        self.table, self.seen = [], {}
        self.classes = self.rhymed = self.lead = None
        self.distinct = False
        self.place = {}                                          # (row, follower line) -> how many lines of its group lie before it

    def set_index(self, ids):
        if ids not in self.seen:
            self.seen[ids] = len(self.table)
            self.table.append(ids)
        if self.seen[ids] > 32767:
            raise ValueError("line_end_ids / templates: more than 32768 distinct id sets")
        return self.seen[ids]

    def fit(self, what, b, spec):
        """Row b's per-line entries of argument `what` as a list no longer than the generation's lines."""
        if isinstance(spec, tuple) and spec and spec[0] == "all":
            spec = [spec[1]] * self.n_lines
        if len(spec) > self.n_lines:
            raise ValueError("%s row %d has %d lines, a generation of length %d holds %d" % (what, b, len(spec), self.length, self.n_lines))
        return spec


def _line_bounds(t, b, spec):
    """Step 1a: row b's line_lengths entries into lo / hi."""
    for l, e in enumerate(t.fit("line_lengths", b, spec)):
        if e is None:
            continue
        pair = (e, e) if _is_int(e) else e
        if not (isinstance(pair, tuple) and len(pair) == 2 and all(_is_int(v) for v in pair)):
            raise ValueError("line_lengths row %d, line %d: an int, a (lo, hi) tuple or None expected, got %r" % (b, l, e))
        a, z = int(pair[0]), int(pair[1])
        if not 0 <= a <= z <= t.cap:
            raise ValueError("line_lengths row %d, line %d: (%d, %d) is not 0 <= lo <= hi <= %d (sent - 2)" % (b, l, a, z, t.cap))
        t.lo[b, l], t.hi[b, l] = a, z


def _line_ends(t, b, spec):
    """Step 1b: row b's line_end_ids entries into set_of."""
    for l, e in enumerate(t.fit("line_end_ids", b, spec)):
        if e is not None:
            ids = _id_set(e, t.V, "line_end_ids row %d, line %d" % (b, l), "end set", "a collection of ids or None")
            t.set_of[b, l] = t.set_index(ids)


def _rhyme_scheme(t, b, sch):
    """Step 2: row b's scheme.  A group's first line (the leader) gets the ids that have a rhyme as a static end set; the others
    (followers) get their leader's line in `lead` and their rank in `place`."""
    if not all(ch == "." or ch.isalpha() for ch in sch):
        raise ValueError("rhyme_scheme row %d: %r holds symbols other than letters and '.'" % (b, sch))
    groups = {}
    for l, ch in enumerate(t.fit("rhyme_scheme", b, sch)):
        if ch != ".":
            groups.setdefault(ch, []).append(l)
    for ch, ls in groups.items():
        if len(ls) < 2:
            continue                                     # a group of one line is unconstrained
        if t.distinct and min(len(k) for k in t.classes) < len(ls):
            raise ValueError("rhyme_scheme row %d: rhyme_distinct and group %r of %d lines, but a rhyme class of %d ids"
                             % (b, ch, len(ls), min(len(k) for k in t.classes)))
        for i, l in enumerate(ls):
            if t.hi[b, l] == 0:
                raise ValueError("rhyme_scheme row %d, line %d: a rhyming line with hi = 0" % (b, l))
            if i == 0:
                ids = t.rhymed if t.set_of[b, l] < 0 else t.rhymed & t.table[t.set_of[b, l]]
                if not ids:
                    raise ValueError("rhyme_scheme row %d, line %d: no id of the line's end set has a rhyme class" % (b, l))
                t.set_of[b, l] = t.set_index(ids)
            else:
                if t.set_of[b, l] >= 0:
                    raise ValueError("rhyme_scheme row %d, line %d: a follower line takes no line_end_ids set of its own" % (b, l))
                t.lead[b, l] = ls[0]
                t.place[b, l] = i


def _sets_need_room(t, b):
    """Step 3: a line that ends on a member of a set holds at least one token."""
    for l in range(t.n_lines):
        if t.set_of[b, l] >= 0 and t.hi[b, l] == 0:
            raise ValueError("line_end_ids row %d, line %d: an end set on a line with hi = 0" % (b, l))


def _line_templates(t, b, spec):
    """Step 4: row b's templates into tmpl, their lengths folded into lo / hi; a template that fixes the line's last column is held
    against the line's end set and, on a follower line, against the rhyme classes."""
    for l, e in enumerate(t.fit("templates", b, spec)):
        if e is None:
            continue
        at = "templates row %d, line %d" % (b, l)
        if not isinstance(e, tuple):
            raise ValueError("%s: a tuple of symbols or None expected, got %r" % (at, e))
        open_ = len(e) > 0 and e[-1] is Ellipsis
        syms = e[:-1] if open_ else e
        k = len(syms)
        if not 1 <= k <= t.cap:
            raise ValueError("%s: %d symbols, not 1 .. %d (sent - 2)" % (at, k, t.cap))
        for c, y in enumerate(syms):
            if y is None:
                continue
            if _is_int(y):
                if not _content_id(int(y), t.V):
                    raise ValueError("%s, column %d: id %d is not a content id below the vocabulary cut" % (at, c, int(y)))
                t.tmpl[b, l, c] = int(y)
            elif isinstance(y, (set, frozenset)) and all(_is_int(v) for v in y):
                t.tmpl[b, l, c] = -2 - t.set_index(_id_set(y, t.V, "%s, column %d" % (at, c), "class"))
            else:
                raise ValueError("%s, column %d: an int, None or a set of ids expected, got %r" % (at, c, y))
        a, z = int(t.lo[b, l]), int(t.hi[b, l])
        if open_:
            if z < k:
                raise ValueError("%s: an open template of %d symbols on a line with hi = %d" % (at, k, z))
            t.lo[b, l] = max(a, k)
        else:
            if not a <= k <= z:
                raise ValueError("%s: a closed template of %d symbols outside the line's bounds (%d, %d)" % (at, k, a, z))
            t.lo[b, l] = t.hi[b, l] = k
        y = syms[-1]
        last = frozenset(int(v) for v in y) if isinstance(y, (set, frozenset)) else None
        if t.set_of[b, l] >= 0 and t.hi[b, l] == k:              # the template's last column is the line's last: the end set's
            members = t.table[t.set_of[b, l]]
            if _is_int(y) and int(y) not in members:
                raise ValueError("%s: the line ends on the given id %d, which is not in its end set" % (at, int(y)))
            if last is not None and not members & last:
                raise ValueError("%s: the last column's class and the line's end set share no id" % at)
        if (b, l) in t.place and t.hi[b, l] == k:                # a follower whose last possible column the template fixes
            if _is_int(y):
                raise ValueError("%s: a follower line of the rhyme scheme ends on the given id %d" % (at, int(y)))
            need = t.place[b, l] + 1 if t.distinct else 1
            if last is not None and any(len(kls & last) < need for kls in t.classes):
                raise ValueError("%s: the last column's class leaves a rhyme class with fewer than %d ids on a follower line" % (at, need))


def _prefix_line(t, b, p):
    """Step 5: row b's prefix p where it stops inside a line: the given columns against the line's template and its hi."""
    l, q = (len(p) - 1) // t.sent, (len(p) - 1) % t.sent
    if not (1 <= q <= t.cap and l < t.n_lines):
        return
    if t.tmpl is not None:
        for c in range(min(q, t.cap)):
            v, y = int(p[l * t.sent + 1 + c]), int(t.tmpl[b, l, c])
            if y >= 0 and v != y:
                raise ValueError("prefix row %d gives id %d at column %d of line %d, its template %d" % (b, v, c, l, y))
            if y <= -2 and v not in t.table[-2 - y]:
                raise ValueError("prefix row %d gives id %d at column %d of line %d, outside its template's class" % (b, v, c, l))
    given = sum(1 for v in p[l * t.sent + 1:] if v != 0)
    if given > t.hi[b, l]:
        raise ValueError("prefix row %d gives %d content tokens of line %d, more than its hi = %d" % (b, given, l, t.hi[b, l]))


def _pack(t):
    """Step 6: the rhyme classes join the sets, last; the sets as bit rows, class_of, and the LineTables."""
    rows_of = None if t.classes is None else [t.set_index(k) for k in t.classes]
    V, sets, class_of = t.V, None, None
    if t.table:
        if V is None:
            V = max(max(s) for s in t.table) + 1
        sets = np.zeros((len(t.table), (V + 31) // 32), np.uint32)
        for i, s in enumerate(t.table):
            for v in s:
                sets[i, v >> 5] |= np.uint32(1 << (v & 31))
    if t.classes is not None:
        class_of = np.full(V, -1, np.int16)
        for i, k in zip(rows_of, t.classes):
            class_of[sorted(k)] = i
    return LineTables(t.lo, t.hi, t.set_of if t.table else None, sets, t.sent, V, t.tmpl, class_of, t.lead, t.distinct)


def check_lines(line_lengths, line_end_ids, rows, length, sent=22, V=None, prefix=None, templates=None, rhyme_scheme=None,
                rhyme_classes=None, rhyme_distinct=False):
    """Validate line-length bounds and line-end id sets on the host, before any device work; returns the packed LineTables, or
    None when both arguments are None (no constraints: the decoders then run the launches of a generation without them).

    A generation of `length` holds n_lines = (length - 1) // sent + 1 lines (those with a content column); line l of row b is
    lyric columns l * sent .. l * sent + sent - 1 and holds up to sent - 2 content tokens.
    line_lengths: a line's entry is an int (exactly that many content tokens), a (lo, hi) tuple or None (unconstrained, the
    same as (0, sent - 2)).  Given as one entry (every line of every row), one list of entries (line by line, for every row; a
    shorter list leaves the later lines unconstrained) or a list with one such list, entry or None per row (the lists, not tuples,
    mark this form).
    line_end_ids: a line's entry is None or a non-empty collection of content ids below the vocabulary cut V (no PAD, none of
    1, 2, 100, 102): the line's last content token is one of them, so the line is not empty and its hi must be >= 1.  Given as
    one set / frozenset (every line), one list of entries, or one list of entries (or None) per row.
    prefix (check_prefix's result, optional): a row whose prefix stops inside a line continues that line under its bounds; given
    content beyond the line's hi raises.  Whole given lines are the caller's text and are not checked.
    templates: a line's entry is None or a tuple of k symbols (1 <= k <= sent - 2), one per content column from column 0 -- an int
    (given: the row writes this content id), None (free) or a set / frozenset of content ids (a class: the column's id is a
    member) -- optionally ending in `...` (Ellipsis: an open template).  A closed template fixes the line's length, its bounds
    become (k, k) and k must lie inside the line's line_lengths bounds; an open one makes lo = max(lo, k) and needs hi >= k.  Given
    as one list of entries (for every row; a shorter list leaves the later lines without a template) or a list with one such list
    or None per row.  Given ids and class members are content ids below V; on a line with an end set whose length the template
    fixes (hi == k) the last symbol must leave a member of the set possible.  A partial prefix line must agree with its line's
    template.  So a column that only classes and end sets constrain always has a live id; only n-gram bans can empty one.
    rhyme_scheme / rhyme_classes / rhyme_distinct: a scheme is a string with one symbol per line -- a letter names the line's
    group, `.` leaves the line alone, a shorter string leaves the later lines alone -- one for every row or a list with one string
    or None per row.  rhyme_classes (required with a scheme) is a list of pairwise disjoint, non-empty sets of content ids below V:
    the ids that have a rhyme, by rhyme.  The first line of a group of two or more is its leader and gets the union of the classes
    as a static end set (intersected with its line_end_ids set, which must leave an id), so it is not empty (hi >= 1); the others
    are followers: they end in the class of the id their leader ended on in that row (include/mmtg_hip.h), with rhyme_distinct not
    on an id an earlier line of the group ended on.  A follower takes no line_end_ids set of its own, needs hi >= 1, and a template
    that fixes its last possible column (hi == k) must leave every class possible there: no given id, and a class symbol that
    meets every rhyme class (with rhyme_distinct in as many ids as the group has lines up to this one).  With rhyme_distinct every
    class has at least as many ids as the largest group has lines; rhyme_distinct without a scheme raises.  A group of one line is
    unconstrained.
    Raises ValueError for bounds outside 0 .. sent - 2, lo > hi, more entries than lines, and any end set, template or scheme that
    breaks the above."""
    if (rhyme_scheme is None) != (rhyme_classes is None):
        raise ValueError("rhyme_scheme and rhyme_classes come together (got %s alone)"
                         % ("rhyme_scheme" if rhyme_classes is None else "rhyme_classes"))
    if rhyme_distinct and rhyme_scheme is None:
        raise ValueError("rhyme_distinct without a rhyme_scheme")
    if line_lengths is None and line_end_ids is None and templates is None and rhyme_scheme is None:
        return None
    if length < 1 or not 3 <= sent <= 257:
        raise ValueError("line constraints need length >= 1 and 3 <= sent <= 257 (got length %d, sent %d)" % (length, sent))
    t = _Draft(rows, length, sent, V, templates is not None)
    lens = _per_row(line_lengths, rows, "line_lengths", lambda e: _is_int(e) or (isinstance(e, tuple) and len(e) == 2),
                    lambda s: any(isinstance(e, list) for e in s))
    ends = _per_row(line_end_ids, rows, "line_end_ids", lambda e: isinstance(e, (set, frozenset)),
                    lambda s: any(isinstance(e, (list, tuple)) and not _is_ids(e) for e in s))
    tmpls = _template_rows(templates, rows)
    schemes = None
    if rhyme_scheme is not None:
        schemes, t.classes, t.distinct = _scheme_rows(rhyme_scheme, rows), _rhyme_classes(rhyme_classes, V), bool(rhyme_distinct)
        if t.n_lines > 128:
            raise ValueError("rhyme_scheme: a generation of %d lines (a scheme serves up to 128)" % t.n_lines)
        t.rhymed = frozenset().union(*t.classes)
        t.lead = np.full((rows, t.n_lines), -1, np.int8)
    for b in range(rows):                                        # row by row, so the sets keep the order they arise in
        _line_bounds(t, b, lens[b])
        _line_ends(t, b, ends[b])
        if schemes is not None:
            _rhyme_scheme(t, b, schemes[b])
        _sets_need_room(t, b)
        _line_templates(t, b, tmpls[b])
        if prefix is not None:
            _prefix_line(t, b, prefix[b])
    return _pack(t)


def _refrain_rows(spec, rows):
    """refrain_scheme as one string per row (_scheme_rows' forms, under its own name in the messages)."""
    try:
        return _scheme_rows(spec, rows)
    except ValueError as e:
        raise ValueError(str(e).replace("rhyme_scheme", "refrain_scheme")) from None


def check_refrain(refrain_scheme, rows, length, sent=22, lines=None, prefix=None, rhyme_scheme=None):
    """Validate refrain_scheme= on the host, before any device work; returns src int8 [rows, n_lines] -- src[b, l] the line whose text
    line l of row b repeats, always < l, or -1 -- or None for refrain_scheme=None.

    A scheme is a string over letters and `.`, one for every row or a list with one string or None per row (rhyme_scheme's forms).
    Character l speaks for lyric line l; lines past the string are free.  Lines with the same letter hold the same text: the first
    line of a letter is its source, an ordinary line under every other rule, and every later line of that letter is a copy of it
    ("AAA": lines 1 and 2 both copy line 0).  `.` and a letter used once mean nothing.  On a copy column -- not a held prefix column,
    not a forced [#START#] / [#EOS#] -- the row writes the id its own history holds at the same column of the source line
    (include/mmtg_hip.h states the rule); no logits, bans or masks are involved, so a copy line is not the model's to shape:
      lines (check_lines' tables of the same generation, optional): a copy line carries no bounds other than its source's or the
        default (0, sent - 2), no end set, no template, and in rhyme_scheme (the argument, optional) no letter other than `.`;
      prefix (check_prefix's lists, optional): a prefix may not end inside a copy line, and a copy line it gives whole must equal its
        source (given too, since it lies before).  Whole given lines are otherwise the caller's text, as prefix columns always are.
    Raises ValueError for symbols other than letters and `.`, a scheme longer than the generation has lines (at most 128), and any
    of the above."""
    if refrain_scheme is None:
        return None
    if length < 1 or not 3 <= sent <= 257:
        raise ValueError("refrain_scheme needs length >= 1 and 3 <= sent <= 257 (got length %d, sent %d)" % (length, sent))
    n_lines, cap = (length - 1) // sent + 1, sent - 2
    if n_lines > 128:
        raise ValueError("refrain_scheme: a generation of %d lines (a scheme serves up to 128)" % n_lines)
    schemes = _refrain_rows(refrain_scheme, rows)
    rhymes = None if rhyme_scheme is None else _scheme_rows(rhyme_scheme, rows)
    src = np.full((rows, n_lines), -1, np.int8)
    own = "refrain_scheme row %d, line %d: a copy line repeats its source (line %d) and is not the model's to shape; it takes no %s"
    for b, sch in enumerate(schemes):
        if not all(ch == "." or ch.isalpha() for ch in sch):
            raise ValueError("refrain_scheme row %d: %r holds symbols other than letters and '.'" % (b, sch))
        if len(sch) > n_lines:
            raise ValueError("refrain_scheme row %d has %d lines, a generation of length %d holds %d" % (b, len(sch), length, n_lines))
        first = {}
        for l, ch in enumerate(sch):
            if ch == ".":
                continue
            if ch not in first:
                first[ch] = l
                continue
            r = src[b, l] = first[ch]
            if lines is not None and l < lines.lo.shape[1]:
                mine, its = (int(lines.lo[b, l]), int(lines.hi[b, l])), (int(lines.lo[b, r]), int(lines.hi[b, r]))
                if lines.tmpl is not None and (lines.tmpl[b, l] != -1).any():
                    raise ValueError(own % (b, l, r, "template"))
                if lines.lead is not None and lines.lead[b, l] >= 0:
                    raise ValueError(own % (b, l, r, "rhyme letter other than '.'"))
                if lines.set_of is not None and lines.set_of[b, l] >= 0:
                    raise ValueError(own % (b, l, r, "end set (line_end_ids, or the leader of a rhyme group)"))
                if mine != (0, cap) and mine != its:
                    raise ValueError(own % (b, l, r, "bounds other than its source's %r or the default (got %r)" % (its, mine)))
            if rhymes is not None and l < len(rhymes[b]) and rhymes[b][l] != ".":
                raise ValueError(own % (b, l, r, "rhyme letter other than '.'"))
        if prefix is not None:
            p = prefix[b]
            l, q = (len(p) - 1) // sent, (len(p) - 1) % sent
            if 1 <= q <= cap and l < n_lines and src[b, l] >= 0:
                raise ValueError("prefix row %d ends inside line %d, a copy line of the refrain scheme (give the line whole, or not at all)"
                                 % (b, l))
            for l in range(n_lines):
                r = int(src[b, l])
                if r >= 0 and len(p) > l * sent + cap:
                    if list(p[l * sent + 1:l * sent + 1 + cap]) != list(p[r * sent + 1:r * sent + 1 + cap]):
                        raise ValueError("prefix row %d gives line %d, a copy line of the refrain scheme, with a text other than its "
                                         "source's (line %d)" % (b, l, r))
    return src


def _bare_tables(rows, length, sent, V, src):
    """LineTables that carry a refrain alone: every line unconstrained."""
    n_lines = (length - 1) // sent + 1
    return LineTables(np.zeros((rows, n_lines), np.uint8), np.full((rows, n_lines), sent - 2, np.uint8), None, None, sent, V, src=src,
                      bare=True)


class Constraints:
    """The checked constraints of a generation's rows: ngram (the n-gram size), prefix (check_prefix's lists, or None) and lines
    (LineTables, or None).  take(idx) / repeat(k) are LineTables' own, on the prefix and the tables together."""

    def __init__(self, ngram, prefix, lines):
        self.ngram, self.prefix, self.lines = ngram, prefix, lines

    def take(self, idx):
        return Constraints(self.ngram, None if self.prefix is None else [self.prefix[i] for i in idx],
                           None if self.lines is None else self.lines.take(idx))

    def repeat(self, k):
        return Constraints(self.ngram, None if self.prefix is None else [p for p in self.prefix for _ in range(k)],
                           None if self.lines is None else self.lines.repeat(k))


def _check_constraints(prefix, no_repeat_ngram_size, line_lengths, line_end_ids, rows, length, sh, what, templates=None,
                       rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, refrain_scheme=None):
    """The constraint arguments of ``begin`` for `rows` rows (`what` names them in messages), checked, as Constraints.  A LineTables
    given as line_lengths is taken as checked (its src included: no refrain_scheme beside it).  A refrain scheme travels in the
    tables' src; given without any line argument, the tables are bare."""
    sent = sh.msl + 2
    ngram = check_ngram(no_repeat_ngram_size, sent)
    pre = None if prefix is None else check_prefix(prefix, rows, length, sent=sent, V=sh.V)
    if not isinstance(line_lengths, LineTables):
        line_lengths = check_lines(line_lengths, line_end_ids, rows, length, sent=sent, V=min(sh.V, 13317), prefix=pre, templates=templates,
                                   rhyme_scheme=rhyme_scheme, rhyme_classes=rhyme_classes, rhyme_distinct=rhyme_distinct)
        src = check_refrain(refrain_scheme, rows, length, sent=sent, lines=line_lengths, prefix=pre, rhyme_scheme=rhyme_scheme)
        if src is not None:
            if line_lengths is None:
                line_lengths = _bare_tables(rows, length, sent, min(sh.V, 13317), src)
            else:
                line_lengths.src = src
    elif (line_lengths.rows != rows or line_end_ids is not None or templates is not None or rhyme_scheme is not None
            or rhyme_classes is not None or rhyme_distinct or refrain_scheme is not None):
        raise ValueError("line tables of %d rows for %s (and no line_end_ids / templates / rhyme_scheme beside them, nor a refrain_scheme)"
                         % (line_lengths.rows, what))
    return Constraints(ngram, pre, line_lengths)


def refrain_without_keywords(keywords, lines):
    """keywords= together with a refrain scheme is the one combination left out: the keyword candidates know nothing of copy lines."""
    if keywords is not None and lines is not None and lines.src is not None:
        raise ValueError("keywords= and refrain_scheme= are not combined: the keyword candidates have no copy columns (ask for one of them)")


# ------------------------------------------------------------------ keywords (BeamDecoder with keywords=; the rule's home is include/mmtg_hip.h)
KW_MAX, KW_LEN = 8, 4
NOT_CONTENT = (0,) + BANNED


class KeywordTables:
    """The checked keywords of `rows` prompts: lists[b] = prompt b's phrases (tuples of ids), phrases int32 [rows, 8, 4] (-1 beyond a
    phrase), lens int8 [rows, 8] (0 beyond a prompt's keywords), K = the most keywords a prompt has and cap = the longest phrase (the
    candidates entry's phrase_cap)."""

    def __init__(self, lists):
        self.lists = [tuple(tuple(int(v) for v in p) for p in row) for row in lists]
        self.rows = len(self.lists)
        self.K = max([len(r) for r in self.lists] + [0])
        self.cap = max([len(p) for r in self.lists for p in r] + [1])
        self.phrases = np.full((self.rows, KW_MAX, KW_LEN), -1, np.int32)
        self.lens = np.zeros((self.rows, KW_MAX), np.int8)
        for b, row in enumerate(self.lists):
            for i, p in enumerate(row):
                self.phrases[b, i, :len(p)] = p
                self.lens[b, i] = len(p)

    def take(self, idx):
        return KeywordTables([self.lists[i] for i in idx])


def _keyword_lists(keywords, rows):
    """keywords as one list of phrases per prompt: it is one list of phrases for all prompts (a phrase: a sequence of ids) or a list
    of `rows` such lists."""
    def is_phrase(e):
        return isinstance(e, (list, tuple, np.ndarray)) and len(e) > 0 and all(_is_int(v) for v in e)

    if not isinstance(keywords, (list, tuple)):
        raise ValueError("keywords must be a list of phrases (id sequences) or one such list per prompt, got %r" % (keywords,))
    if all(is_phrase(e) for e in keywords):
        return [list(keywords) for _ in range(rows)]
    if all(isinstance(e, (list, tuple)) for e in keywords) and len(keywords) == rows:
        return [list(e) for e in keywords]
    if any(isinstance(e, (list, tuple, np.ndarray)) and len(e) == 0 for e in keywords):
        raise ValueError("keywords: an empty phrase (a keyword is 1..%d content ids)" % KW_LEN)
    raise ValueError("keywords must be a list of phrases (id sequences) or one such list for each of the %d prompts" % rows)


def _windows(ids, phrase):
    n, L = len(ids), len(phrase)
    return any(tuple(ids[i:i + L]) == tuple(phrase) for i in range(n - L + 1))


def check_keywords(keywords, n_prompts, nb, V, sent=22, prefix=None):
    """Validate keywords= on the host, before any device work, and pack them: a KeywordTables (None for keywords=None; a KeywordTables
    is taken as checked).  keywords: one list of phrases for all prompts or one list per prompt; a phrase is 1 .. 4 content ids (not
    0, 1, 2, 100, 102, below min(V, 13317)) and no longer than a line holds (sent - 2).  A prompt has at most 8 phrases, all
    distinct, none a contiguous sub-phrase of another, and nb * (nb + K) <= 256 (K the most keywords a prompt has): one merge
    workgroup has one candidate per thread.  prefix (check_prefix's lists): one per prompt; a keyword that already lies in a prompt's
    prefix is no error -- the history includes the prefix, so it is met from the start and its slot is dead."""
    if keywords is None:
        return None
    if isinstance(keywords, KeywordTables):
        if keywords.rows != n_prompts:
            raise ValueError("keyword tables of %d prompts for %d prompts" % (keywords.rows, n_prompts))
        tabs = keywords
    else:
        lists = _keyword_lists(keywords, n_prompts)
        cut = min(int(V), 13317)
        for b, row in enumerate(lists):
            if len(row) > KW_MAX:
                raise ValueError("keywords of prompt %d: %d phrases, at most %d" % (b, len(row), KW_MAX))
            for i, p in enumerate(row):
                if not isinstance(p, (list, tuple, np.ndarray)) or not 1 <= len(p) <= min(KW_LEN, sent - 2):
                    raise ValueError("keywords of prompt %d, phrase %d: a keyword is 1..%d content ids, got %r" % (b, i, min(KW_LEN, sent - 2), p))
                for v in p:
                    if not _is_int(v) or int(v) in NOT_CONTENT or not 0 <= int(v) < cut:
                        raise ValueError("keywords of prompt %d, phrase %d: %r is not a content id below %d" % (b, i, v, cut))
            ps = [tuple(int(v) for v in p) for p in row]
            for i, p in enumerate(ps):
                for k, q in enumerate(ps):
                    if i < k and p == q:
                        raise ValueError("keywords of prompt %d: phrases %d and %d are the same" % (b, i, k))
                    if i != k and len(p) < len(q) and _windows(q, p):
                        raise ValueError("keywords of prompt %d: phrase %d lies inside phrase %d" % (b, i, k))
        tabs = KeywordTables(lists)
    if int(nb) * (int(nb) + tabs.K) > 256:
        raise ValueError("keywords: %d beams x (%d beams + %d keywords) candidates exceed 256 (one merge workgroup)" % (nb, nb, tabs.K))
    if prefix is not None:
        if len(prefix) != n_prompts:
            raise ValueError("keywords: prefix of %d rows for %d prompts" % (len(prefix), n_prompts))
    return tabs


def keyword_met_mask(ids, phrases):
    """Per phrase: it occurs in the id sequence `ids` as a contiguous window."""
    ids = [int(v) for v in ids]
    return [_windows(ids, p) for p in phrases]


def keywords_met(ids, phrases):
    """How many of the phrases occur in `ids` as contiguous windows."""
    return int(sum(keyword_met_mask(ids, phrases)))


def keyword_bank(ids, phrases):
    """bank(s) of include/mmtg_hip.h for the sequence s = ids: the lengths of the met phrases plus prog(s), the largest m with
    1 <= m < len_i over the unmet phrases i such that s ends in phrase_i[0..m) (0 if none).  Host only, from the definition."""
    s = [int(v) for v in ids]
    met = keyword_met_mask(s, phrases)
    bank = sum(len(p) for p, m in zip(phrases, met) if m)
    prog = 0
    for p, m in zip(phrases, met):
        if not m:
            for k in range(1, len(p)):
                if k <= len(s) and tuple(s[len(s) - k:]) == tuple(p[:k]):
                    prog = max(prog, k)
    return bank + prog


def keyword_select(cands, nb):
    """The keyword merge's selection on the host.  cands: (base, bank, token) in candidate order o (parent-major, slot-minor).  A NaN
    base is -inf; live means base > -inf.  A live candidate's r is the number of live candidates of its bank before it by (base
    descending, o ascending); the live ones are ordered by (r ascending, bank descending), the dead ones follow in o order.  Returns
    the first nb as (o, base fp32, bank, token)."""
    keyed = []
    for o, (base, bank, tok) in enumerate(cands):
        base = np.float32(base)
        keyed.append((o, np.float32(-np.inf) if np.isnan(base) else base, int(bank), int(tok)))
    live = [c for c in keyed if c[1] > -np.inf]
    dead = [c for c in keyed if not c[1] > -np.inf]
    rank = {}
    for bank in {c[2] for c in live}:
        for r, c in enumerate(sorted((c for c in live if c[2] == bank), key=lambda c: (-float(c[1]), c[0]))):
            rank[c[0]] = r
    live.sort(key=lambda c: (rank[c[0]], -c[2]))
    return (live + dead)[:nb]
