"""Drop-in for the reference's generation helpers (src/generate.py:64-145).

``sample_sequence`` keeps the reference's signature (including the misspelt
``repitition_penalty``), its forced [#START#]/[#EOS#] cadence, sticky PAD and the
lagging return value.  The model call is the HIP engine; the greedy setting
(top_k=1, top_p=0) post-processes logits with the fused HIP kernel
(mmtg_logits_process_argmax); the stochastic setting uses mmtg_logits_process_sample (the reference's
penalty / temperature / bans / top-k / top-p, then one draw by inverse CDF with a uniform from torch's generator --
torch.multinomial's own stream cannot be reproduced outside torch; the distribution is the reference's).
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from . import hip
from .constraints import (BANNED, GUIDANCE_OFF, WARP_OFF, Constraints, _check_constraints, check_mirostat, check_modality_guidance, check_warp, check_contrastive, check_groups, check_keywords, check_prefix, check_stochastic, refrain_without_keywords,
                          sequence_scores)
from .decode import BeamDecoder, ContrastiveDecoder, GreedyDecoder, GuidedDecoder, ModalityGuidedDecoder, StochasticBeamDecoder, _keywords_need_beams
from .data import encode_line_end, encode_prefix, encode_rhyme_classes, encode_template  # noqa: F401  (public: the opening lines / the line-end sets / the line templates / the rhyme classes of generate_samples / generate_beams)

SENT_SLOT = 22  # generate.py:118-121


def top_k_top_p_filtering(logits, top_k=0, top_p=0.0, filter_value=-float("Inf")):
    """Top-k / nucleus filter on a 1-D logits tensor, in place (generate.py:64-94)."""
    assert logits.dim() == 1
    top_k = min(top_k, logits.size(-1))
    if top_k > 0:
        kth = torch.topk(logits, top_k)[0][..., -1, None]
        logits[logits < kth] = filter_value
    if top_p > 0.0:
        sorted_logits, sorted_indices = torch.sort(logits, descending=True)
        cum = torch.cumsum(F.softmax(sorted_logits, dim=-1), dim=-1)
        remove = cum > top_p
        remove[..., 1:] = remove[..., :-1].clone()
        remove[..., 0] = 0
        logits[sorted_indices[remove]] = filter_value
    return logits


def _check_tokenizer(tokenizer):
    if tokenizer is None:
        return
    got = tuple(tokenizer.convert_tokens_to_ids(t) for t in ("[#START#]", "[#EOS#]", "[UNK]", "[SEP]"))
    if got != BANNED:
        raise ValueError("tokenizer special ids %s differ from the reference vocabulary's %s" % (got, BANNED))


def _cached_decoder(model, start_input, length, guided=False, blocks=2):
    """The KV-cached, graph-replayed decoder for this call, or None when the call is not the one the reference's
    generate.py makes (an MMTG in inference mode on the GPU -- possibly inside the nn.DataParallel wrapper of generate.py:191 --
    started from the single [#START#] token, generate.py:207-209).  MMTG_SAMPLE_RERUN=1 forces the prefix re-run loop.
    guided: a GuidedDecoder of one prompt (two rows) instead; with blocks > 2 a ModalityGuidedDecoder of one prompt (blocks rows)."""
    from .model import MMTG
    m = getattr(model, "module", model)
    if not isinstance(m, MMTG) or m.train_flag or not m._flat.is_cuda or os.environ.get("MMTG_SAMPLE_RERUN"):
        return None
    if m.training:
        # a model left in train() mode: the prefix re-run loop follows the module mode (dropout, torch.multinomial draws);
        # the cached decoder never applies dropout and draws from its own uniform stream, so it only serves eval() models
        return None
    t = np.asarray(start_input["targets"]).reshape(-1)
    sh = m.shapes
    if t.shape[0] != 1 or int(t[0]) != 1 or length < 1 or sh.P + length + 1 > sh.NP:
        return None
    cache = m.__dict__.setdefault("_sample_decoders", {})
    key = (m._flat.data_ptr(), int(length)) + (("guided",) if guided else ()) + (("blocks", blocks) if guided and blocks > 2 else ())
    dec = cache.get(key)
    if dec is None:
        cache.clear()                       # one decoder (KV caches + graphs) at a time
        dec = cache[key] = (ModalityGuidedDecoder(m, 1, blocks, max_len=int(length)) if guided and blocks > 2
                            else GuidedDecoder(m, 1, max_len=int(length)) if guided else GreedyDecoder(m, max_batch=1, max_len=int(length)))
    return dec


def sample_sequence(model, start_input, length, tokenizer, temperature=1.0, top_k=30, top_p=0.0,
                    repitition_penalty=1.0, device="cuda", *, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0,
                    mirostat_tau=0.0, mirostat_eta=0.1, guidance_scale=1.0, negative_input=None, image_guidance_scale=1.0,
                    text_guidance_scale=1.0):
    """generate.py:97-145.  When the call is the reference's own (see _cached_decoder) the loop runs on the KV-cached decoder:
    one captured token step replayed per position instead of a full forward over the growing prefix per token; the returned
    list is what the reference loop returns (the sequence before the last model call's append).  Greedy ids are the same as
    the re-run loop's bit for bit in the f32 mode (tests/test_decode_gpu.py).
    min_p / typical_p / epsilon_cutoff / eta_cutoff (keyword only, so the reference's positional signature stands): min-p, locally
    typical, epsilon and eta sampling behind top_k / top_p (constraints.check_warp, include/mmtg_hip.h); any of them on samples.
    mirostat_tau / mirostat_eta (keyword only; constraints.check_mirostat, include/mmtg_hip.h): Mirostat v2 behind all of them, the
    sequence's surprise state carried from draw to draw; mirostat_tau > 0 samples.
    guidance_scale / negative_input (keyword only; constraints.check_guidance, include/mmtg_hip.h): classifier-free guidance,
    transformers' argument of that name.  Any scale but 1 runs the model on start_input and on negative_input (the same keys; default:
    start_input with img_embs and r_embs zeroed) and selects from lu + guidance_scale * (lc - lu) of their log-softmaxed logits: on
    the cached path a GuidedDecoder of one prompt, in the re-run loop a second forward and mmtg_decode_guidance on the two last rows.
    guidance_scale=1 (the default) is the call without the arguments; negative_input beside it is a ValueError.
    image_guidance_scale / text_guidance_scale (keyword only; constraints.check_modality_guidance, include/mmtg_hip.h): per-modality
    guidance, as generate_samples takes it.  One scale other than 1 among the three is the guided call above with that branch's
    negative (start_input without its images, or without its texts); two or three run a ModalityGuidedDecoder of one prompt on the
    cached path.  The prefix re-run loop does not take them: there two or three scales other than 1 are a ValueError that says so.
    negative_input replaces the negative of guidance_scale only."""
    _check_tokenizer(tokenizer)
    branches, scales = check_modality_guidance(guidance_scale, image_guidance_scale, text_guidance_scale)
    if "u" not in branches and negative_input is not None:
        raise ValueError("negative_input needs a guidance_scale other than 1 (1 is the unguided call)")
    guided = len(branches) > 0
    zero = {"u": ("img_embs", "r_embs"), "i": ("img_embs",), "t": ("r_embs",)}
    negatives = [negative_input if b == "u" and negative_input is not None else
                 {k: (np.zeros_like(np.asarray(v)) if k in zero[b] else v) for k, v in start_input.items()} for b in branches]
    scale = scales[0] if guided else GUIDANCE_OFF       # (one running branch: GuidedDecoder's case, whichever branch it is)
    negative_input = negatives[0] if guided else None
    warp = check_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    warp_kw = {} if warp == WARP_OFF else dict(zip(("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"), warp))
    tau, eta = check_mirostat(mirostat_tau, mirostat_eta)
    miro_kw = {"mirostat_tau": tau, "mirostat_eta": eta} if tau > 0.0 else {}
    dec = _cached_decoder(model, start_input, length, guided=guided, blocks=1 + len(branches))
    if dec is None and len(branches) > 1:
        raise ValueError("%d guidance scales other than 1 need the cached decoder: the prefix re-run loop runs one negative (an eval() "
                         "MMTG on the GPU, started from [#START#], without MMTG_SAMPLE_RERUN)" % len(branches))
    if dec is not None:
        m = getattr(model, "module", model)
        batch = {k: torch.as_tensor(np.asarray(v)).unsqueeze(0) for k, v in start_input.items() if k not in ("targets", "rating")}
        if len(branches) > 1:
            negs = [{k: torch.as_tensor(np.asarray(neg[k])).unsqueeze(0) for k in batch} for neg in negatives]
            ids = dec.generate(batch, negs, int(length), branches, scales, temperature=temperature, repitition_penalty=repitition_penalty,
                               top_k=int(top_k), top_p=float(top_p), **warp_kw, **miro_kw)
            return dec.reference_return(ids[0].tolist(), int(length), sent=m.shapes.msl + 2)
        if guided:
            neg = {k: torch.as_tensor(np.asarray(negative_input[k])).unsqueeze(0) for k in batch}
            ids = dec.generate(batch, neg, int(length), scale, temperature=temperature, repitition_penalty=repitition_penalty,
                               top_k=int(top_k), top_p=float(top_p), **warp_kw, **miro_kw)
            return dec.reference_return(ids[0].tolist(), int(length), sent=m.shapes.msl + 2)
        ids = dec.generate(batch, int(length), temperature=temperature, repitition_penalty=repitition_penalty,
                           top_k=int(top_k), top_p=float(top_p), **warp_kw, **miro_kw)
        return dec.reference_return(ids[0].tolist(), int(length), sent=m.shapes.msl + 2)
    inputs = {}
    for k, v in start_input.items():
        if k == "targets":
            inputs[k] = torch.tensor(np.asarray(v), dtype=torch.long, device=device).unsqueeze(0)
        else:
            inputs[k] = torch.tensor(np.asarray(v), dtype=torch.float32, device=device).unsqueeze(0)
    neg_inputs = None
    if guided:      # the negative prompt beside the prompt: its own conditioning, the same growing targets
        neg_inputs = {k: torch.tensor(np.asarray(negative_input[k]), dtype=torch.float32, device=device).unsqueeze(0)
                      for k in start_input if k != "targets"}
    generated = inputs["targets"]
    greedy = top_k == 1 and top_p == 0.0 and not warp_kw and not miro_kw
    mu = torch.full((1,), 2.0 * tau, dtype=torch.float32, device=device) if miro_kw else None
    nxt = torch.zeros(1, dtype=torch.long, device=device)
    glen = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.no_grad():
        for i in range(length):
            if i > 0 and (i + 2) % SENT_SLOT == 0:
                inputs["targets"] = torch.cat((inputs["targets"], torch.tensor([[2]], device=device)), dim=-1)
                continue
            if i > 0 and (i + 2) % SENT_SLOT == 1:
                inputs["targets"] = torch.cat((inputs["targets"], torch.tensor([[1]], device=device)), dim=-1)
                continue
            _, _, outputs = model.forward(inputs)
            generated = inputs["targets"]
            if guided:
                # the guided scores of the two last rows take the raw logits' place (columns past the cut are never read)
                cond = outputs[0, -1, :].float().clone()       # (a copy: the engine's next forward may write the same buffer)
                _, _, outputs_u = model.forward(dict(neg_inputs, targets=generated))
                uncond = outputs_u[0, -1, :].float().contiguous()
                guided_row = torch.zeros(1, cond.shape[0], dtype=torch.float32, device=cond.device)
                hip.decode_guidance(cond, uncond, cond.shape[0], min(cond.shape[0], 13317), scale, guided_row, 1)
                outputs = guided_row.view(1, 1, -1)
            if greedy:
                row = outputs[0, -1, :]
                glen.fill_(generated.shape[1])
                hip.logits_process_argmax(row, row.shape[0], min(row.shape[0], 13317), generated.contiguous(),
                                          generated.shape[1], glen, temperature, repitition_penalty, nxt, 1)
                next_token = nxt.view(1, 1).clone()
            else:
                row = outputs[0, -1, :]
                glen.fill_(generated.shape[1])
                u = torch.rand(1, device=device).clamp_(max=1.0 - 2.0 ** -24)
                if miro_kw:
                    hip.logits_process_sample_mirostat(row, row.shape[0], min(row.shape[0], 13317), generated.contiguous(),
                                                       generated.shape[1], glen, temperature, repitition_penalty, top_k, top_p, u, nxt, 1,
                                                       tau, eta, mu, **warp_kw)
                else:
                    draw = hip.logits_process_sample_warp if warp_kw else hip.logits_process_sample
                    draw(row, row.shape[0], min(row.shape[0], 13317), generated.contiguous(),
                         generated.shape[1], glen, temperature, repitition_penalty, top_k, top_p, u, nxt, 1, **warp_kw)
                next_token = nxt.view(1, 1).clone()
            inputs["targets"] = torch.cat((generated, next_token), dim=-1)
    return generated.tolist()[0]


# ------------------------------------------------------------------ the sampling product path (generate.py:205-235)
def postprocess_tokens(preds):
    """The reference's cut rules and detokenisation of one sampled token list (generate.py:222-235):
    cut after the 10th [#EOS#] when there are at least ten and no [SEP] before the last one, else after the first
    [SEP], else append one; then join, drop [SEP] / [PAD] / [#START#], turn [#EOS#] into the full-width comma and strip
    trailing commas.  (An all-special list leaves an empty string; the reference would raise IndexError there.)"""
    preds = list(preds)
    eos = [i for i, v in enumerate(preds) if v == "[#EOS#]"]
    if len(eos) >= 10 and "[SEP]" not in preds[:eos[-1]]:
        preds = preds[:eos[9] + 1] + ["[SEP]"]
    elif "[SEP]" in preds:
        preds = preds[:preds.index("[SEP]") + 1]
    else:
        preds = preds + ["[SEP]"]
    text = "".join(preds).replace("[SEP]", "").replace("[PAD]", "").replace("[#START#]", "").replace("[#EOS#]", "，")
    while text and text[-1] == "，":
        text = text[:-1]
    return text


def encode_keywords(tokenizer, words, vocab_cut=13317):
    """The phrases of keywords= (constraints.check_keywords) from words, e.g. encode_keywords(tokenizer, ["月光", "海"]): one tuple of
    ids per word, one character one token.  A word is 1 .. 4 characters; an empty or longer word raises ValueError, as does a
    character the tokenizer does not know ([UNK]), whitespace, a special token, PAD or an id at or above the generation's
    vocabulary cut."""
    if isinstance(words, str):
        raise ValueError("keywords are a list of words, got the string %r" % (words,))
    phrases = []
    for w in words:
        if not isinstance(w, str) or not 1 <= len(w) <= 4:
            raise ValueError("keyword %r: a keyword is a word of 1..4 characters" % (w,))
        ids = []
        for ch in w:
            v = -1 if ch.isspace() else int(tokenizer.convert_tokens_to_ids(ch))
            if v in (0, 1, 2, 100, 102) or not 0 <= v < vocab_cut:
                raise ValueError("keyword %r: character %r maps to id %d, not a content id below %d" % (w, ch, v, vocab_cut))
            ids.append(v)
        phrases.append(tuple(ids))
    return phrases


def _stack_rows(rows):
    """rows (a list of dataset items, or a dict of stacked arrays) as one tensor per model input, a prompt per row."""
    keys = ("topic_ids", "tpw_attention_mask", "tpw_type_ids", "topic_emb", "img_embs", "r_embs")
    if isinstance(rows, dict):
        return {k: torch.as_tensor(np.asarray(rows[k])) for k in keys}
    return {k: torch.as_tensor(np.stack([np.asarray(r[k]) for r in rows])) for k in keys}


def without_experience(rows):
    """The default negative prompt of classifier-free guidance: `rows` (as generate_samples takes them) stacked, with the images and
    texts of the experience (img_embs, r_embs) zeroed and the topic kept -- what the model would write about the topic alone."""
    out = _stack_rows(rows)
    out["img_embs"], out["r_embs"] = torch.zeros_like(out["img_embs"]), torch.zeros_like(out["r_embs"])
    return out


def without_images(rows):
    """The negative prompt of image_guidance_scale: `rows` stacked, with the images (img_embs) zeroed and the texts and the topic kept."""
    out = _stack_rows(rows)
    out["img_embs"] = torch.zeros_like(out["img_embs"])
    return out


def without_texts(rows):
    """The negative prompt of text_guidance_scale: `rows` stacked, with the texts (r_embs) zeroed and the images and the topic kept."""
    out = _stack_rows(rows)
    out["r_embs"] = torch.zeros_like(out["r_embs"])
    return out


def _chunks(stacked, cons, size, dev, copies=1):
    """The prompts of `stacked`, each `copies` times in a row, cut into decoder batches of exactly `size` rows on `dev`: yields
    (batch, the rows' Constraints, the number of real rows).  The decoder's batch is fixed, so the last chunk is padded by repeating
    its first row."""
    total = stacked["topic_ids"].shape[0] * copies
    for lo in range(0, total, size):
        n = min(total, lo + size) - lo
        idx = [r // copies for r in range(lo, lo + n)] + [lo // copies] * (size - n)
        yield {k: v[idx].to(dev) for k, v in stacked.items()}, cons.take(idx), n


def guided_chunk_size(max_batch, blocks, rows):
    """How many prompts' rows a guided chunk of generate_samples holds: max_batch // blocks (blocks = 1 + the running negatives), at
    least 1, at most the `rows` there are."""
    return max(1, min(int(max_batch) // int(blocks), int(rows)))


def rank_scored(scored, rank_by):
    """One prompt's (text, logprob_sum, n_tokens) triples best first: by the sum ("sum") or by sum / max(n_tokens, 1) ("mean", so a
    sample without a counted token ranks by its sum, 0).  The sort is stable: equal keys keep their draw order."""
    if rank_by not in ("sum", "mean"):
        raise ValueError('rank_by must be "sum", "mean" or None, got %r' % (rank_by,))
    key = (lambda t: t[1]) if rank_by == "sum" else (lambda t: t[1] / max(t[2], 1))
    return sorted(scored, key=key, reverse=True)


def generate_samples(model, rows, tokenizer, n_samples=10, length=None, temperature=1.1, top_k=10, top_p=0.7,
                     repetition_penalty=1.5, max_batch=256, generator=None, decoder=None, prefixes=None, no_repeat_ngram_size=0,
                     line_lengths=None, line_end_ids=None, templates=None, rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False,
                     return_scores=False, rank_by=None, keywords=None, refrain_scheme=None, *, min_p=0.0, typical_p=1.0,
                     epsilon_cutoff=0.0, eta_cutoff=0.0, mirostat_tau=0.0, mirostat_eta=0.1, guidance_scale=1.0, negative_rows=None,
                     image_guidance_scale=1.0, text_guidance_scale=1.0):
    """n_samples texts per prompt (generate.sh's loop, generate.py:205-235) on the batched, graph-replayed decoder:
    every prompt is replicated over n_samples rows, rows are decoded max_batch at a time with the device-side
    top-k / top-p sampler (one uniform per row and position from `generator`), each row is cut back to what
    sample_sequence would have returned (the sequence before the last model call's append) and post-processed.

    rows: list of dataset items (dicts with topic_ids / tpw_* / topic_emb / img_embs / r_embs, numpy or tensors) or a dict of
    stacked arrays.  Returns a list (one entry per prompt) of lists of n_samples strings.
    prefixes (optional): one list of opening lyric ids per prompt (encode_prefix, decode.check_prefix); every sample of the prompt
    continues it, and its text includes the given lines.
    no_repeat_ngram_size (optional, decode.check_ngram): n > 0 keeps every row from writing a content n-gram it already holds.
    line_lengths / line_end_ids (optional, decode.check_lines; one per prompt or one for all): bounds on every line's number of
    tokens and sets (encode_line_end) a line's last token comes from; every sample of a prompt follows its prompt's.
    templates (optional, decode.check_lines; one list of line templates per prompt or one for all): given characters, free columns
    and id classes for the opening columns of a line (encode_template), e.g. an acrostic
    templates=[encode_template(tokenizer, c + "…") for c in "春夏秋冬"].
    rhyme_scheme / rhyme_classes / rhyme_distinct (optional, decode.check_lines; one scheme per prompt or one for all): lines that
    end on one rhyme, e.g. rhyme_scheme="AABB", rhyme_classes=encode_rhyme_classes(tokenizer, ["光忙香", "天年前"]); every sample
    chooses its own rhymes.  rhyme_distinct=True keeps a line from ending on the character an earlier line of its group ended on.
    refrain_scheme (optional, constraints.check_refrain; one scheme per prompt or one for all): lines that repeat a line, e.g.
    refrain_scheme="AB.A" makes line 3 the text of line 0 again, whatever the sample wrote there -- also under no_repeat_ngram_size.
    A copy line takes no bounds, end set, template or rhyme letter of its own.
    return_scores: each prompt's entry is a list of (text, logprob_sum, n_tokens) instead -- the sum of the model's own token
    log-probabilities (raw logits: no penalty, no temperature, no bans, so comparable across sampling settings;
    GreedyDecoder.begin, return_logprobs) over the columns of the returned text that decode.chosen_mask counts, past the prompt's
    prefix, and how many those are.  Columns a constraint decided (a template's given id, a full line's PAD) count, at the model's
    log-probability of that id; the samples of a prompt share their constraints, so ranking among them is fair.
    rank_by: "sum" or "mean" (sum / max(n_tokens, 1)) orders a prompt's samples best first (stable) and implies return_scores.
    The texts are the strings, from the same `generator` state, of the call without the two arguments.
    keywords: refused (ValueError): a lyric that contains given words needs a search over beams -- generate_beams(keywords=).
    min_p / typical_p / epsilon_cutoff / eta_cutoff (keyword only; constraints.check_warp, include/mmtg_hip.h): min-p, locally typical,
    epsilon and eta sampling, transformers' arguments of those names, behind top_k / top_p and under every constraint above, e.g.
    typical_p=0.9, min_p=0.05 with top_k=0, top_p=0.  At their defaults the call is the call without them.
    mirostat_tau / mirostat_eta (keyword only; constraints.check_mirostat, include/mmtg_hip.h): Mirostat v2, llama.cpp's arguments of
    those names, behind all of the above: mirostat_tau=2.0 with top_k=0, top_p=0 holds every sample's surprise near 2 bits per drawn
    character.  Each of the n_samples rows of a prompt has its own state.  mirostat_tau=0 (the default) is the call without them.
    guidance_scale / negative_rows (keyword only; constraints.check_guidance, include/mmtg_hip.h, decode.GuidedDecoder): classifier-free
    guidance, transformers' argument of that name: guidance_scale=3.0 makes every sample follow its prompt's images and texts more
    closely than the model alone would, by sharpening each step's distribution against that of a negative prompt -- negative_rows (rows
    as above, one per prompt or one for all; default without_experience(rows): the topic alone).  Every other argument works as
    before, on the guided scores; the scores of return_scores stay the model's own log-probabilities under the real prompt.  A
    guided chunk holds max_batch // 2 rows beside their negatives.  guidance_scale=1 (the default) is the call without the
    arguments; negative_rows beside it is a ValueError.
    image_guidance_scale / text_guidance_scale (keyword only; constraints.check_modality_guidance, include/mmtg_hip.h,
    decode.ModalityGuidedDecoder): a scale per modality, e.g. image_guidance_scale=3.0, text_guidance_scale=1.5 -- follow the photos
    more, the captions a little more.  Each scale other than 1 runs a negative of its own beside the prompt, in the order
    guidance_scale (without_experience, or negative_rows), image_guidance_scale (without_images), text_guidance_scale (without_texts),
    and each step selects from lc + sum_k (s_k - 1) (lc - l_k) of the log-softmaxed logits.  One scale other than 1 is the guided
    call above with that negative: image_guidance_scale=s alone is guidance_scale=s, negative_rows=without_images(rows), bit for bit.
    With K - 1 running negatives a chunk holds max_batch // K rows.  Both at 1 (the default) is the call without them."""
    _keywords_need_beams(keywords)
    branches, scales = check_modality_guidance(guidance_scale, image_guidance_scale, text_guidance_scale)
    if "u" not in branches and negative_rows is not None:
        raise ValueError("negative_rows needs a guidance_scale other than 1 (1 is the unguided call)")
    guided, K = len(branches) > 0, 1 + len(branches)
    warp_kw = dict(zip(("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"), check_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)))
    warp_kw["mirostat_tau"], warp_kw["mirostat_eta"] = check_mirostat(mirostat_tau, mirostat_eta)
    if rank_by is not None and rank_by not in ("sum", "mean"):
        raise ValueError('rank_by must be "sum", "mean" or None, got %r' % (rank_by,))
    scoring = bool(return_scores) or rank_by is not None
    eng = model.engine()
    sh = eng.sh
    length = sh.max_seq_length if length is None else length
    n_prompts = len(rows["topic_ids"]) if isinstance(rows, dict) else len(rows)
    cons = _check_constraints(prefixes, no_repeat_ngram_size, line_lengths, line_end_ids, n_prompts, length, sh, "%d prompts" % n_prompts,
                              templates, rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme)
    stacked = _stack_rows(rows)
    if guided:
        make = {"u": without_experience, "i": without_images, "t": without_texts}
        neg_list = []
        for b in branches:
            neg = _stack_rows(negative_rows) if b == "u" and negative_rows is not None else make[b](rows)
            n_neg = neg["topic_ids"].shape[0]
            if n_neg == 1 and n_prompts > 1:
                neg = {k: v.expand(n_prompts, *v.shape[1:]) for k, v in neg.items()}
            elif n_neg != n_prompts:
                raise ValueError("negative_rows: one row per prompt (%d) or one for all, got %d" % (n_prompts, n_neg))
            neg_list.append(neg)
        bsz = guided_chunk_size(max_batch, K, n_prompts * n_samples)
        if K == 2:      # one running branch, whichever: the two-row decoder and its kernels
            dec = (decoder if isinstance(decoder, GuidedDecoder) and not isinstance(decoder, ModalityGuidedDecoder)
                   and decoder.n_prompts == bsz else GuidedDecoder(model, bsz, max_len=length))
        else:
            dec = (decoder if isinstance(decoder, ModalityGuidedDecoder) and (decoder.n_prompts, decoder.blocks) == (bsz, K)
                   else ModalityGuidedDecoder(model, bsz, K, max_len=length))
        negs = [_chunks(neg, cons, bsz, eng.dev, copies=n_samples) for neg in neg_list]     # (the prompts' chunks, row for row)
    else:
        bsz = min(max_batch, n_prompts * n_samples)
        dec = decoder if decoder is not None and decoder.B == bsz else GreedyDecoder(model, max_batch=bsz, max_len=length)
    texts = []
    for chunk, c, n in _chunks(stacked, cons, bsz, eng.dev, copies=n_samples):
        lead = ((length,) if not guided else (next(negs[0])[0], length, scales[0]) if K == 2 else
                ([next(g)[0] for g in negs], length, branches, scales))
        ids = dec.generate(chunk, *lead, temperature=temperature,
                           repitition_penalty=repetition_penalty,
                           top_k=top_k, top_p=top_p, generator=generator, prefix=c.prefix, no_repeat_ngram_size=c.ngram,
                           line_lengths=c.lines, return_logprobs=scoring, **warp_kw)
        if scoring:
            ids, lp = ids[0].cpu().numpy(), ids[1].cpu().numpy()
            upto = len(GreedyDecoder.reference_return(ids[0].tolist(), length, sent=sh.msl + 2))        # 1 + the last model call
            sums, counts = sequence_scores(ids, lp, sent=sh.msl + 2, upto=upto,
                                           prefix_lens=None if c.prefix is None else [len(p) for p in c.prefix])
        else:
            ids = ids.cpu().numpy()
        for r in range(n):
            seq = GreedyDecoder.reference_return(ids[r].tolist(), length, sent=sh.msl + 2)
            text = postprocess_tokens(tokenizer.convert_ids_to_tokens(seq))
            texts.append((text, float(sums[r]), int(counts[r])) if scoring else text)
    out = [texts[i * n_samples:(i + 1) * n_samples] for i in range(n_prompts)]
    return [rank_scored(e, rank_by) for e in out] if rank_by is not None else out


def score_sequences(model, rows, ids, max_batch=256):
    """Per-token log-probabilities of GIVEN lyric ids under their prompts: float32 numpy [n, 1 + length].  rows: as
    generate_samples; ids: one row of 1 + length lyric ids per prompt in decode.check_prefix's layout (what GreedyDecoder.generate
    and BeamDecoder.generate return, or encode_prefix of written lines padded to whole rows).  Column j holds the log-probability
    the model's raw logits give ids[b][j] after ids[b][:j]; column 0 and the forced [#START#] / [#EOS#] columns hold 0
    (decode.sequence_scores sums the columns that count).
    This is the decoder's scoring mode (GreedyDecoder.begin: the ids as a prefix that covers every row whole, return_logprobs):
    teacher forcing through the token-step kernels that generate, chunked and padded to the batch like generate_samples.  The cost
    is `length` token steps per chunk of max_batch rows, not one batched pass: it is built to agree with the generator's numerics
    (the values a generation reported for its own ids come back within rounding), not for bulk evaluation -- that is
    MMTGTrainer.evaluate."""
    eng = model.engine()
    sh = eng.sh
    n_prompts = len(rows["topic_ids"]) if isinstance(rows, dict) else len(rows)
    given = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    if given.ndim != 2 or given.shape[0] != n_prompts or given.shape[1] < 2:
        raise ValueError("ids must be [%d prompts, 1 + length] (got shape %s)" % (n_prompts, given.shape))
    length = given.shape[1] - 1
    pre = check_prefix(given, n_prompts, length, sent=sh.msl + 2, V=min(sh.V, 13317))
    if any(len(p) != length + 1 for p in pre):
        raise ValueError("ids must cover every row whole (no -1 padding)")
    bsz = min(max_batch, n_prompts)
    dec = GreedyDecoder(model, max_batch=bsz, max_len=length)
    out = []
    for chunk, c, n in _chunks(_stack_rows(rows), Constraints(0, pre, None), bsz, eng.dev):
        back, lp = dec.generate(chunk, length, prefix=c.prefix, return_logprobs=True)
        if not np.array_equal(back[:n].cpu().numpy(), np.asarray(c.prefix[:n])):
            raise RuntimeError("score_sequences: the decoder changed a given id")
        out.append(lp[:n].cpu().numpy())
    return np.concatenate(out)


def generate_beams(model, rows, tokenizer, num_beams=4, length=None, temperature=1.1, repetition_penalty=1.5, max_batch=256,
                   return_all=False, prefixes=None, no_repeat_ngram_size=0, line_lengths=None, line_end_ids=None, templates=None,
                   rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, return_ids=False, num_beam_groups=1,
                   diversity_penalty=0.0, best_per_group=False, keywords=None, return_met=False, refrain_scheme=None):
    """Beam search per prompt on the batched, graph-replayed decoder (BeamDecoder): prompts are decoded max_batch // num_beams at
    a time, every beam is cut back to what sample_sequence would have returned (GreedyDecoder.reference_return) and
    post-processed as generate_samples does.  rows: as generate_samples.  Returns one string per prompt (its best beam), or with
    return_all=True one list per prompt of num_beams (text, score) pairs, best first (score: the sum of the fp32 log-probabilities
    of the processed logits at the positions the model chose; see BeamDecoder).  prefixes: as generate_samples (the prefix
    positions add nothing to a score).  no_repeat_ngram_size: as generate_samples, on every beam's own history.  line_lengths /
    line_end_ids / templates: as generate_samples, shared by a prompt's beams (a full line and a given column add nothing to a
    score).  rhyme_scheme / rhyme_classes / rhyme_distinct: as generate_samples; every beam rhymes with its own earlier lines.
    return_ids (with return_all): (text, score, ids) triples, ids the beam's 1 + length lyric ids -- a row score_sequences takes, which
    gives the beam the model's raw token log-probabilities (the score here changes with temperature, penalty and every ban).
    num_beam_groups / diversity_penalty: diverse beam search (BeamDecoder.begin): G groups of num_beams / G beams, a later group
    lowered by the penalty for every earlier group's beam that takes the same content id at the same step; scores stay the
    unpenalised sums, so the list of return_all is still best first over all groups.  best_per_group=True returns one list per
    prompt of G entries in group order, each the best hypothesis of its group as (text, score), or (text, score, ids) with
    return_ids; it excludes return_all.
    keywords: words the lyric should contain, each at a place of the model's choice -- encode_keywords(tokenizer, ["月光", "海"]), one
    list for all prompts or one list per prompt (constraints.check_keywords; BeamDecoder.begin).  A prompt's beams are then ordered
    by (keywords met descending, score descending), so the text returned is the best hypothesis that holds the most keywords.  The
    search is best effort: return_met=True (with return_all) appends the number of keywords met to each beam's tuple.  Not together
    with num_beam_groups > 1.
    refrain_scheme: as generate_samples; every beam repeats its own earlier line, e.g.
    generate_beams(..., refrain_scheme="AB.A", no_repeat_ngram_size=3).  Not together with keywords (ValueError)."""
    G, lam = check_groups(num_beams, num_beam_groups, diversity_penalty)
    BeamDecoder._keywords_alone(keywords, G)
    if return_met and (keywords is None or not return_all):
        raise ValueError("return_met reports, per beam of return_all, the keywords it holds: give keywords= and return_all=True")
    if best_per_group and return_all:
        raise ValueError("best_per_group returns one hypothesis per group, return_all every beam: ask for one of them")
    eng = model.engine()
    sh = eng.sh
    length = sh.max_seq_length if length is None else length
    n_prompts = len(rows["topic_ids"]) if isinstance(rows, dict) else len(rows)
    cons = _check_constraints(prefixes, no_repeat_ngram_size, line_lengths, line_end_ids, n_prompts, length, sh, "%d prompts" % n_prompts,
                              templates, rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme)
    refrain_without_keywords(keywords, cons.lines)
    kw = check_keywords(keywords, n_prompts, num_beams, sh.V, sh.msl + 2, prefix=cons.prefix)
    per = max(1, min(max_batch // num_beams, n_prompts))
    dec = BeamDecoder(model, per, num_beams, max_len=length)
    out = []
    done = 0
    for chunk, c, n in _chunks(_stack_rows(rows), cons, per, eng.dev):
        if kw is None:
            ids, scores, group = dec.generate(chunk, length, temperature=temperature, repitition_penalty=repetition_penalty, prefix=c.prefix,
                                              no_repeat_ngram_size=c.ngram, line_lengths=c.lines, num_beam_groups=G, diversity_penalty=lam,
                                              return_groups=True)
        else:                      # (the chunk's prompts' keywords; the padding rows repeat the chunk's first prompt, as _chunks does)
            idx = list(range(done, done + n)) + [done] * (per - n)
            ids, scores, met = dec.generate(chunk, length, temperature=temperature, repitition_penalty=repetition_penalty, prefix=c.prefix,
                                            no_repeat_ngram_size=c.ngram, line_lengths=c.lines, keywords=kw.take(idx), return_met=True)
            group, met = torch.zeros_like(met), met.cpu().numpy()
        done += n
        ids, scores, group = ids.cpu().numpy(), scores.cpu().numpy(), group.cpu().numpy()
        for r in range(n):
            beams = []
            for k in range(num_beams):
                seq = GreedyDecoder.reference_return(ids[r, k].tolist(), length, sent=sh.msl + 2)
                beams.append((postprocess_tokens(tokenizer.convert_ids_to_tokens(seq)), float(scores[r, k]))
                             + ((ids[r, k].tolist(),) if return_ids else ()) + ((int(met[r, k]),) if return_met else ()))
            if best_per_group:         # (best first, so a group's first place is its best)
                out.append([beams[int(np.argmax(group[r] == g))] for g in range(G)])
            else:
                out.append(beams if return_all else beams[0][0])
    return out


def generate_contrastive(model, rows, tokenizer, top_k=4, penalty_alpha=0.6, length=None, temperature=1.1, repetition_penalty=1.5,
                         max_batch=256, prefixes=None, no_repeat_ngram_size=0, line_lengths=None, line_end_ids=None, templates=None,
                         rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, refrain_scheme=None, return_ids=False,
                         keywords=None, num_beam_groups=1):
    """Contrastive search per prompt on the batched, graph-replayed decoder (ContrastiveDecoder; Su et al. 2022): at every step the
    model's top_k most probable characters are tried, and the one kept is the best by (1 - penalty_alpha) * probability -
    penalty_alpha * (the largest cosine between its last-layer hidden state and those of the lyric so far).  One deterministic
    lyric per prompt, at about the cost of a top_k-beam search; penalty_alpha=0 (or top_k=1) is greedy decoding.  Prompts are
    decoded max_batch // top_k at a time; every lyric is cut back to what sample_sequence would have returned
    (GreedyDecoder.reference_return) and post-processed as generate_samples does.  rows: as generate_samples.
    Returns one (text, score) pair per prompt, or with return_ids=True (text, score, ids): score is the sum of the processed
    log-probabilities of the chosen tokens (a beam score's scale), ids the 1 + length lyric ids -- a row score_sequences takes.
    prefixes, no_repeat_ngram_size, line_lengths / line_end_ids, templates, rhyme_scheme / rhyme_classes / rhyme_distinct,
    refrain_scheme: as generate_beams -- the rules act on the candidates, so the search chooses among characters they allow.
    keywords= and num_beam_groups > 1 are refused with a ValueError that says why (ContrastiveDecoder); the model's raw token
    log-probabilities of a returned lyric come from score_sequences on its ids."""
    ContrastiveDecoder._refuse(keywords=keywords, num_beam_groups=num_beam_groups)
    k, alpha = check_contrastive(top_k, penalty_alpha)
    eng = model.engine()
    sh = eng.sh
    length = sh.max_seq_length if length is None else length
    n_prompts = len(rows["topic_ids"]) if isinstance(rows, dict) else len(rows)
    cons = _check_constraints(prefixes, no_repeat_ngram_size, line_lengths, line_end_ids, n_prompts, length, sh, "%d prompts" % n_prompts,
                              templates, rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme)
    per = max(1, min(max_batch // k, n_prompts))
    dec = ContrastiveDecoder(model, per, k, max_len=length)
    out = []
    for chunk, c, n in _chunks(_stack_rows(rows), cons, per, eng.dev):
        ids, scores = dec.generate(chunk, length, penalty_alpha=alpha, temperature=temperature, repitition_penalty=repetition_penalty,
                                   prefix=c.prefix, no_repeat_ngram_size=c.ngram, line_lengths=c.lines)
        ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        for r in range(n):
            seq = GreedyDecoder.reference_return(ids[r].tolist(), length, sent=sh.msl + 2)
            out.append((postprocess_tokens(tokenizer.convert_ids_to_tokens(seq)), float(scores[r]))
                       + ((ids[r].tolist(),) if return_ids else ()))
    return out


def generate_stochastic_beams(model, rows, tokenizer, num_samples=4, seed=0, length=None, temperature=1.1, repetition_penalty=1.5,
                              max_batch=256, prefixes=None, no_repeat_ngram_size=0, line_lengths=None, line_end_ids=None, templates=None,
                              rhyme_scheme=None, rhyme_classes=None, rhyme_distinct=False, refrain_scheme=None, return_ids=False,
                              return_perturbed=False, keywords=None, num_beam_groups=1, diversity_penalty=0.0, return_logprobs=False,
                              top_k=1, top_p=0.0, generator=None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0,
                              mirostat_tau=0.0, mirostat_eta=0.1):
    """num_samples DIFFERENT lyrics per prompt by stochastic beam search on the batched, graph-replayed decoder (StochasticBeamDecoder;
    Kool, van Hoof and Welling 2019): an exact sample without replacement from the distribution generate_samples draws from at
    top_k=0, top_p=0 -- the processed logits: repetition penalty, temperature, bans and every line rule -- where generate_samples
    draws its n_samples independently and may return one lyric several times.  The cost is about that of a num_samples-beam search.
    Prompts are decoded max_batch // num_samples at a time; a prompt's noise depends on seed, its index among `rows` and the beam
    slot, not on max_batch.  Every lyric is cut back to what sample_sequence would have returned (GreedyDecoder.reference_return)
    and post-processed as generate_samples does.  rows: as generate_samples.
    Returns, per prompt, a list of num_samples tuples in draw order (the first is an ordinary sample): (text, score), score the sum
    of the processed log-probabilities of the lyric's tokens (a beam score's scale); return_ids=True appends the 1 + length lyric
    ids (a row score_sequences takes), return_perturbed=True then the sample's perturbed value (0 for the first, non-increasing).
    A prompt whose rules leave fewer than num_samples different lyrics returns only those it has.
    prefixes, no_repeat_ngram_size, line_lengths / line_end_ids, templates, rhyme_scheme / rhyme_classes / rhyme_distinct,
    refrain_scheme: as generate_contrastive -- the rules act on the candidates, so the samples come from what they allow.
    keywords=, num_beam_groups > 1, a diversity penalty, return_logprobs, sampling top_k / top_p / generator, min_p / typical_p /
    epsilon_cutoff / eta_cutoff and Mirostat are refused with a ValueError that says why (StochasticBeamDecoder)."""
    StochasticBeamDecoder._refuse(keywords=keywords, num_beam_groups=num_beam_groups, return_logprobs=return_logprobs,
                                  diversity_penalty=diversity_penalty, top_k=top_k, top_p=top_p, generator=generator, min_p=min_p,
                                  typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, mirostat_tau=mirostat_tau,
                                  mirostat_eta=mirostat_eta)
    nb, seed = check_stochastic(num_samples, seed)
    eng = model.engine()
    sh = eng.sh
    length = sh.max_seq_length if length is None else length
    n_prompts = len(rows["topic_ids"]) if isinstance(rows, dict) else len(rows)
    cons = _check_constraints(prefixes, no_repeat_ngram_size, line_lengths, line_end_ids, n_prompts, length, sh, "%d prompts" % n_prompts,
                              templates, rhyme_scheme, rhyme_classes, rhyme_distinct, refrain_scheme)
    per = max(1, min(max_batch // nb, n_prompts))
    dec = StochasticBeamDecoder(model, per, nb, max_len=length)
    out, first = [], 0
    for chunk, c, n in _chunks(_stack_rows(rows), cons, per, eng.dev):
        ids, scores, gum = dec.generate(chunk, length, seed=seed, temperature=temperature, repitition_penalty=repetition_penalty,
                                        prefix=c.prefix, no_repeat_ngram_size=c.ngram, line_lengths=c.lines, first_prompt=first)
        first += per
        ids, scores, gum = ids.cpu().numpy(), scores.cpu().numpy(), gum.cpu().numpy()
        for r in range(n):
            got = []
            for s in range(nb):
                if not gum[r, s] > -np.inf:
                    continue
                seq = GreedyDecoder.reference_return(ids[r, s].tolist(), length, sent=sh.msl + 2)
                got.append((postprocess_tokens(tokenizer.convert_ids_to_tokens(seq)), float(scores[r, s]))
                           + ((ids[r, s].tolist(),) if return_ids else ()) + ((float(gum[r, s]),) if return_perturbed else ()))
            out.append(got)
    return out
