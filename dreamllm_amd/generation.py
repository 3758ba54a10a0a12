"""Host side of text generation for `DreamLLMForCausalMLM`: the protocols of the reference's generation loops, each written once.

`greedy_generate`, `sample_generate`, `generate` and `generate_interleaved` on the model are argument handling plus one call of a
driver here (`greedy_decode`, `sampled_decode`, `beam_decode`, `interleaved_decode`).  A driver either runs a `decode` session (fast path: one hipGraph replay per
token, the host only reads flags between chunks of replays -- `run_chunked`) or re-enters the model forward per token like the
reference (`ModelStepper`).  The drivers differ in how a token is chosen (arg-max / `ops.sample_logits` / `ops.beam_step`);
position ids, the ragged-prompt protocol, the stopping-criterion rule and the session cache are shared.  Everything above the
drivers is index arithmetic on whatever device its arguments live on, so it runs (and is tested) without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import ops


def left_pad_position_ids(attention_mask):
    """Mask-aware position ids as HF generate computes them (`prepare_inputs_for_generation`, modeling_dreamllm.py:1527-1533): a
    valid token's position is the number of valid tokens before it; pad positions get 1."""
    return (attention_mask.long().cumsum(-1) - 1).masked_fill(attention_mask == 0, 1)


def check_left_padded(attention_mask, who="prefill"):
    """-> (start, lens) [B] of a LEFT-padded mask [B, S]: row b's valid tokens are `start[b] : S`.  Right-padded or holey masks
    raise: a decode session appends new tokens at slot S, so a right-padded row would need a hole between its prompt and them."""
    am = attention_mask != 0
    S = am.shape[1]
    lens = am.sum(-1)
    start = S - lens
    if not bool(((torch.arange(S, device=am.device)[None] >= start[:, None]) == am).all()):
        raise ValueError(f"{who}: attention_mask must be LEFT-padded (one run of valid tokens ending at the last prompt position); "
                         "right-padded ragged prompts go through forced tokens (`pad_token_id`)")
    return start, lens


def split_ragged_prompt(input_ids, pad_token_id, max_new_tokens, attention_mask=None):
    """The `pad_token_id` protocol of the reference loop (omni/eval/language_eval/modeling_dreamllm.py:47-109): `input_ids` is
    RIGHT-padded with `pad_token_id`, the prefill covers the shortest prompt (`min_prompt_size`), and rows still inside their
    prompt are teacher-forced (`input_text_mask`, :72,93-94).

    -> (prompt, n_new, tokens, forced, forced_mask): prompt = input_ids[:, :s0] with s0 the shortest prompt; n_new tokens follow
    it; `tokens` [B, S + max_new_tokens] is the result buffer (prompts, then `pad_token_id`); `forced` / `forced_mask` are its
    columns from s0 on and their "given by the prompt" flags.  `pad_token_id=None`: a dense batch, (input_ids, max_new_tokens,
    None, None, None)."""
    if pad_token_id is None:
        return input_ids, max_new_tokens, None, None, None
    if attention_mask is not None:
        raise ValueError("pass either pad_token_id (right-padded ragged prompts) or attention_mask (left-padded), not both")
    B, S = input_ids.shape
    dev = input_ids.device
    text_mask = input_ids != pad_token_id
    plen = text_mask.sum(-1)
    if not bool((text_mask == (torch.arange(S, device=dev)[None] < plen[:, None])).all()):
        raise ValueError("pad_token_id protocol: prompts must be right-padded")
    s0 = int(plen.min())
    total = S + max_new_tokens
    tokens = torch.full((B, total), pad_token_id, dtype=torch.long, device=dev)
    tokens[:, :S] = input_ids
    fmask = torch.zeros(B, total, dtype=torch.bool, device=dev)
    fmask[:, :S] = text_mask
    return input_ids[:, :s0], total - s0, tokens, tokens[:, s0:], fmask[:, s0:]


def _join(input_ids, prompt, tokens, new):
    """Result layout: the ragged protocol's `tokens` buffer with `new` written after the common prompt (columns past a trimmed
    `new` stay `pad_token_id`), else cat([input_ids, new])."""
    if tokens is None:
        return torch.cat([input_ids, new], dim=1)
    s0 = prompt.shape[1]
    tokens[:, s0:s0 + new.shape[1]] = new
    return tokens


def stopped(criteria, ids, scores):
    """True when any stopping criterion (callable (ids, scores) -> bool | BoolTensor) fires; a tensor counts when `.all()`."""
    for c in criteria:
        r = c(ids, scores)
        if bool(r.all()) if isinstance(r, torch.Tensor) else bool(r):
            return True
    return False


class ModelStepper:
    """The reference's way to decode (`fast=False`): re-enter the model forward per token with `past_key_values`.

    Construction runs the prefill of `prompt` [B, S] (`attention_mask`: LEFT padding, mask-aware position ids); `logits` holds the
    last-position logits [B * repeat, V] of the latest forward.  `repeat` > 1 (beam search) repeats every prompt's cache, mask and
    logits that many times after the prefill (row r = b * repeat + beam)."""

    def __init__(self, model, prompt, images=None, attention_mask=None, repeat=1):
        position_ids = left_pad_position_ids(attention_mask) if attention_mask is not None else None
        out = model(input_ids=prompt, images=images, attention_mask=attention_mask, position_ids=position_ids, use_cache=True,
                    return_dict=True)
        self.model, self.past, self.mask, self.logits = model, out.past_key_values, attention_mask, out.logits[:, -1]
        if repeat > 1:
            self.past = tuple((k.repeat_interleave(repeat, 0), v.repeat_interleave(repeat, 0)) for k, v in self.past)
            self.mask = attention_mask.repeat_interleave(repeat, 0) if attention_mask is not None else None
            self.logits = self.logits.repeat_interleave(repeat, 0)

    def step(self, tok, parents=None):
        """Feed `tok` [rows] as the next token of every row -> last-position logits [rows, V].  The mask grows by a column of ones
        and the token's position is its row's valid length - 1; `parents` [rows] (beam search) first reorders the cache rows."""
        if parents is not None:
            self.past = tuple((k.index_select(0, parents), v.index_select(0, parents)) for k, v in self.past)
        pos = None
        if self.mask is not None:
            self.mask = torch.cat([self.mask, self.mask.new_ones(self.mask.shape[0], 1)], dim=1)
            pos = (self.mask.long().sum(-1) - 1)[:, None]
        out = self.model(input_ids=tok[:, None], past_key_values=self.past, attention_mask=self.mask, position_ids=pos,
                         use_cache=True, return_dict=True)
        self.past, self.logits = out.past_key_values, out.logits[:, -1]
        return self.logits


def decode_weights(model):
    """The FP8 decode-weight holder set by `model.quantize_decode_weights` (`decode.DecodeWeightsFP8`), or None: what every fast
    path passes to its session as `weights=`."""
    return getattr(model, "_decode_weights", None)


def cached_session(model, key, factory):
    """The model's one decode session (`model._decode_session = (key, session)`, assignable to None to drop it): equal calls reuse
    it and its captured graph, a call of another kind or shape replaces it.  `key`: a tuple starting with the session kind; a
    decode-weight holder on the model is made part of it here, so setting or dropping the holder replaces the session too."""
    held_weights = decode_weights(model)
    if held_weights is not None:
        key = key + (("weights", held_weights),)
    held = getattr(model, "_decode_session", None)
    if held is None or held[0] != key:
        held = (key, factory())
        model._decode_session = held
    return held[1]


def run_chunked(session, n_new, per_step, halted):
    """Host loop of a prefilled session: `session.generate` until `n_new` tokens exist (the prefill's included) or `halted(n,
    chunk)` -- called after the prefill (chunk None) and after every chunk [rows, m] -- says stop.  -> tokens produced.
    `per_step` (stopping criteria see every token): one replay per check; otherwise the flags are read between chunks of 16."""
    n = 1
    halt = halted(n, None)
    while not halt and n < n_new:
        m = 1 if per_step else min(16, n_new - n)
        chunk = session.generate(m)
        n += m
        halt = halted(n, chunk)
    return n


def _vocab(model, vocab_limit, attention_mask):
    """Ids the token choice runs over.  "auto": 32000 for the language-eval protocols (the reference loop's own slice), the whole
    vocabulary when an `attention_mask` selects HF-generate semantics (HF's search does not slice)."""
    if vocab_limit == "auto":
        vocab_limit = None if attention_mask is not None else 32000
    return min(int(vocab_limit), model.config.vocab_size) if vocab_limit is not None else model.config.vocab_size


@torch.no_grad()
def greedy_decode(model, input_ids, max_new_tokens, images=None, fast=None, use_graph=True, attention_mask=None, pad_token_id=None,
                  vocab_limit="auto"):
    """Body of `DreamLLMForCausalMLM.greedy_generate`: arg-max over the first `vocab_limit` ids, no eos rule."""
    B = input_ids.shape[0]
    V = _vocab(model, vocab_limit, attention_mask)
    if fast is None:
        fast = B <= 8
    prompt, n_new, tokens, forced, fm = split_ragged_prompt(input_ids, pad_token_id, max_new_tokens, attention_mask)
    if fast:
        from .decode import GreedyDecodeSession
        max_len = prompt.shape[1] + n_new + 1
        sess = cached_session(model, ("greedy", B, max_len, use_graph, V),
                              lambda: GreedyDecodeSession(model, B, max_len, use_graph=use_graph, vocab_limit=V,
                                                          weights=decode_weights(model)))
        first = sess.prefill(prompt, images=images, attention_mask=attention_mask, forced_tokens=forced, forced_mask=fm)
        new = torch.cat([first[:, None], sess.generate(n_new - 1)], dim=1)
    else:
        stepper = ModelStepper(model, prompt, images, attention_mask)
        new = []
        for i in range(n_new):
            nxt = stepper.logits[:, :V].argmax(-1)
            if fm is not None:
                nxt = torch.where(fm[:, i], forced[:, i], nxt)
            new.append(nxt)
            if i + 1 < n_new:
                stepper.step(nxt)
        new = torch.stack(new, 1)
    return _join(input_ids, prompt, tokens, new)


@torch.no_grad()
def sampled_decode(model, input_ids, max_new_tokens, temperature, top_k, top_p, vocab_limit, images, attention_mask, pad_token_id,
                   seed, fast, use_graph, eos=None, pad=0, stopping_criteria=None, greedy=False):
    """Shared body of `sample_generate` / `generate` without beams: every token is one `ops.sample_logits` launch (temperature,
    top-k, top-p, the draw keyed by `seed`, teacher forcing, HF's finished-row rule).  `greedy`: u = 0 for every draw (with top-k
    1: the first arg-max, as argmax picks it).  The output ends at the first step where every row has emitted `eos` or a
    stopping criterion, called with (ids so far, that step's fp32 logits), fires."""
    B = input_ids.shape[0]
    dev = input_ids.device
    V = _vocab(model, vocab_limit, attention_mask)
    if fast is None:
        fast = B <= 8
    prompt, n_new, tokens, forced, fm = split_ragged_prompt(input_ids, pad_token_id, max_new_tokens, attention_mask)
    eos = -1 if eos is None else int(eos)
    crit = list(stopping_criteria or [])
    if fast:
        from .decode import SampledDecodeSession
        max_len = prompt.shape[1] + n_new + 1
        sess = cached_session(
            model, ("sample", B, max_len, use_graph, V, temperature, top_k, top_p, eos, int(pad), greedy),
            lambda: SampledDecodeSession(model, B, max_len, temperature, top_k, top_p, eos=eos, pad=pad, use_graph=use_graph,
                                         vocab_limit=V, fixed_u=0.0 if greedy else None, weights=decode_weights(model)))
        first = sess.prefill(prompt, images=images, attention_mask=attention_mask, forced_tokens=forced, forced_mask=fm, seed=seed)
        parts, all_finished = [first[:, None]], False

        def halted(n, chunk):
            nonlocal all_finished
            if chunk is not None:
                parts.append(chunk)
            if crit and stopped(crit, torch.cat([input_ids] + parts, 1), sess.first_logits if chunk is None else sess.logits):
                return True
            all_finished = eos >= 0 and bool(sess.finished.all())  # with eos alone this is the only host read, once per chunk
            return all_finished

        done = run_chunked(sess, n_new, bool(crit), halted)
        new = torch.cat(parts, 1)
        if all_finished:
            hit = (new == eos).int().argmax(1)  # first eos per row (every row has one: all are finished)
            done = int(hit.max()) + 1
        new = new[:, :done]
    else:
        stepper = ModelStepper(model, prompt, images, attention_mask)
        out_buf = torch.zeros(n_new, B, dtype=torch.long, device=dev)
        ftok = forced.t().contiguous() if forced is not None else None
        fmk = fm.t().contiguous() if fm is not None else None
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
        seed_t = torch.tensor([seed], dtype=torch.long, device=dev)
        step_t = torch.zeros(1, dtype=torch.long, device=dev)
        tok = torch.empty(B, dtype=torch.long, device=dev)
        uni = torch.zeros(B, dtype=torch.float32, device=dev) if greedy else None
        done = n_new
        for i in range(n_new):
            scores = stepper.logits.float()
            ops.sample_logits(scores, temperature, top_k, top_p, vocab_limit=V, seed=seed_t, step=step_t, out_tokens=out_buf,
                              force_tok=ftok, force_mask=fmk, eos=eos, pad=pad, finished=finished if eos >= 0 else None,
                              tok_out=tok, advance_step=True, uniforms=uni)
            if (crit and stopped(crit, torch.cat([input_ids, out_buf[: i + 1].t()], 1), scores)) or \
                    (eos >= 0 and bool(finished.all())):
                done = i + 1
                break
            if i + 1 < n_new:
                stepper.step(tok.clone())  # a copy: the kernel overwrites `tok` in the next step
        new = out_buf[:done].t()
    return _join(input_ids, prompt, tokens, new)


@torch.no_grad()
def beam_decode(model, input_ids, max_new_tokens, nb, nrs, length_penalty, early_stopping, images, attention_mask, eos, pad,
                stopping_criteria, fast, use_graph):
    """Beam search (INTEGRATION.md "Beam search"): every step's candidate selection and bookkeeping is one `dllm_beam_step` launch.
    Fast path (B * nb <= 8 unless `fast=False`): `decode.BeamDecodeSession`, one graph replay per token over a copy-free KV cache;
    the host reads the done flags between chunks of 16 replays, or after every replay when stopping criteria are given.
    Otherwise the model forward is re-entered per token with the cache reordered by `index_select`, as the reference does.
    Criteria are called as crit(ids [B * nb, S + n] running beams, None)."""
    B, S = input_ids.shape
    eos = -1 if eos is None else int(eos)
    max_length = S + max_new_tokens
    fast = (fast is None or bool(fast)) and B * nb <= 8
    crit = list(stopping_criteria or [])
    running = input_ids.repeat_interleave(nb, 0)

    def criteria_stop(state, i):
        """Advance the running beams by step i (only criteria read them) and ask the criteria."""
        nonlocal running
        if not crit:
            return False
        running = torch.cat([running.index_select(0, state.parents[i].long()), state.tokens[i][:, None]], 1)
        return stopped(crit, running, None)

    if fast:
        from .decode import BeamDecodeSession
        sess = cached_session(
            model, ("beam", B, nb, max_length + 1, use_graph, eos, pad, length_penalty, early_stopping, max_new_tokens),
            lambda: BeamDecodeSession(model, B, nb, max_length + 1, eos=eos, pad=pad, length_penalty=length_penalty,
                                      early_stopping=early_stopping, max_new=max_new_tokens, use_graph=use_graph,
                                      weights=decode_weights(model)))
        sess.prefill(input_ids, images=images, attention_mask=attention_mask)
        state = sess.beam
        n = run_chunked(sess, max_new_tokens, bool(crit), lambda n, chunk: criteria_stop(state, n - 1) or bool(state.done.all()))
    else:
        stepper = ModelStepper(model, input_ids, images, attention_mask, repeat=nb)
        state = ops.BeamState(B, nb, max_new_tokens + 1, input_ids.device)
        for i in range(max_new_tokens):
            ops.beam_step(stepper.logits.float(), state, eos=eos, pad=pad, length_penalty=length_penalty,
                          early_stopping=early_stopping, max_new=max_new_tokens)
            n = i + 1
            if criteria_stop(state, i) or n == max_new_tokens or bool(state.done.all()):
                break
            stepper.step(state.tok.clone(), parents=state.parents[i].long())  # a copy: the kernel overwrites `tok` in the next step
    return ops.beam_finalize(state, n, input_ids, nrs, max_length, eos, pad, length_penalty)


# ---------------------------------------------------------------------------------------------- interleaved text and images
@dataclass
class InterleavedOutput:
    """Result of `DreamLLMForCausalMLM.generate_interleaved`: `sequences[b]` 1-D LongTensor (row b's prompt without its padding, then
    everything generated, layout ids in place); `images[b]` the row's images, fp32 [3, H, W] in [0, 1], in document order;
    `image_positions[b]` the index of each <dream_start> in `sequences[b]`."""
    sequences: list
    images: list
    image_positions: list


class InterleaveLayout(NamedTuple):
    """Ids and lengths of an image in a document, as the reference's data builder lays it out (omni/data/builders/
    builder_dreamllm.py:110-128): <dream_start> [n_query placeholder ids] <dream_end> <im_start> [n_patch <im_patch> ids] <im_end>."""
    trigger: int
    placeholder: int
    dream_end: int
    im_start: int
    im_patch: int
    im_end: int
    n_query: int
    n_patch: int

    @property
    def block_len(self):
        """Layout tokens that follow an emitted <dream_start>."""
        return self.n_query + 1 + 1 + self.n_patch + 1

    def ids_after_trigger(self):
        return [self.placeholder] * self.n_query + [self.dream_end, self.im_start] + [self.im_patch] * self.n_patch + [self.im_end]


def assemble_row(prompt, segments, layout):
    """One row's document: `prompt` (1-D LongTensor) followed, per segment (tokens, image), by the chosen `tokens` (1-D; with `image`
    the last of them is the <dream_start> the row emitted) and, with `image`, the layout ids the runtime supplied.
    -> (sequence 1-D LongTensor, [index of each <dream_start>])."""
    parts, positions, n = [prompt], [], int(prompt.numel())
    for tokens, image in segments:
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=prompt.device).reshape(-1)
        parts.append(tokens)
        n += int(tokens.numel())
        if image:
            if tokens.numel() == 0 or int(tokens[-1]) != layout.trigger:
                raise ValueError("assemble_row: an image segment must end with the trigger id")
            positions.append(n - 1)
            parts.append(torch.tensor(layout.ids_after_trigger(), dtype=torch.long, device=prompt.device))
            n += layout.block_len
    return torch.cat(parts), positions


def assemble_interleaved(prompts, phases, layout):
    """Row sequences of a batch from what the decode session recorded.  `prompts`: B 1-D LongTensors; `phases`: one (tokens, taken,
    image) per phase -- `tokens` LongTensor [n, B] are the per-step tokens of the phase (the first from the phase's opening logits,
    then one per graph replay), `taken[b]` is the row's park step (how many of them belong to row b: up to and including the token
    it parked on; 0 for a row that was not alive), `image[b]` says that the row parked on <dream_start> and got its image block.
    -> (sequences, image_positions)."""
    seqs, poss = [], []
    for b, prompt in enumerate(prompts):
        segs = [(tokens[: int(taken[b]), b], bool(image[b])) for tokens, taken, image in phases if int(taken[b]) > 0]
        seq, pos = assemble_row(prompt, segs, layout)
        seqs.append(seq)
        poss.append(pos)
    return seqs, poss


def interleave_layout(model):
    sp = model.config.special_tokens2ids_dict["additional_special_tokens"]
    return InterleaveLayout(trigger=sp["<dream_start>"], placeholder=sp[model._dream_patch_token], dream_end=sp["<dream_end>"],
                            im_start=sp["<im_start>"], im_patch=sp["<im_patch>"], im_end=sp["<im_end>"],
                            n_query=model.model.dream_embedding.embed_len, n_patch=model.model.clip_vision_embedding.embed_len)


def trigger_room(layout, prompt_len, max_new_tokens, max_positions):
    """Largest index c (0-based, among the new tokens) at which a row may still emit <dream_start>: the trigger and the two blocks
    must fit `max_new_tokens` (c + 1 + block_len <= max_new_tokens) and the position ids (<im_end> sits at position prompt_len + c +
    block_len < max_positions).  Negative: never."""
    return min(max_new_tokens - 1 - layout.block_len, max_positions - 1 - layout.block_len - prompt_len)


def clip_pixels(model, image):
    """Decoded image fp32 [1, 3, H, W] in [0, 1] -> CLIP pixel values on the device (`ops.image_to_clip`), sized and normalised by
    the CLIP embedding's processor config.  The kernel resizes the shorter side to the size it then crops to, as OpenAI CLIP's
    processor does (`size["shortest_edge"] == crop_size`); a processor whose two sizes differ raises."""
    proc = model.model.clip_vision_embedding.processor
    crop = proc.crop_size
    crop = (crop["height"], crop["width"]) if isinstance(crop, dict) else (int(crop), int(crop))
    edge = getattr(proc, "size", None)
    edge = edge.get("shortest_edge", crop[0]) if isinstance(edge, dict) else (crop[0] if edge is None else int(edge))
    if crop[0] != crop[1] or edge != crop[0]:
        raise ValueError(f"clip_pixels: the CLIP processor resizes to {edge} and crops to {crop}; the hand-off needs one square size")
    return ops.image_to_clip(image, crop[0], proc.image_mean, proc.image_std, out_dtype=model.dtype)


_MIX = 0x9E3779B97F4A7C15  # odd 64-bit constant (2^64 / golden ratio): spreads small indices over the whole key space


def _i64(x):
    return (x + 2 ** 63) % 2 ** 64 - 2 ** 63


def phase_seed(seed, phase):
    """Philox key of the token draws of phase `phase` (int64): seed + phase * _MIX, wrapped."""
    return _i64(int(seed) + int(phase) * _MIX)


def image_generator(seed, row, index):
    """CPU generator of the `index`-th image of row `row` (latents and ancestral noise of its denoising loop), derived from the
    call's seed: an image's noise depends on (seed, row, index) alone -- not on the order in which a path synthesises the images
    of a batch, and not on the other rows."""
    return torch.Generator().manual_seed(_i64(int(seed) ^ ((1 + int(row) + 64 * (1 + int(index))) * _MIX)) & (2 ** 63 - 1))


def _image_event(model, layout, append, synthesize):
    """A row has emitted <dream_start>: `append(embeds [1, L, d]) -> last hidden states [1, L, d]` runs a block as the row's next L
    positions.  [<dream_start>, queries, <dream_end>] -> the queries' hidden states -> `synthesize` -> the image -> CLIP pixel values
    -> [<im_start>, patch embeddings, <im_end>].  -> (image fp32 [3, H, W], fp32 logits [V] at <im_end>)."""
    dq = model.model.prepare_dream_queries_with_special_token(1).to(model.dtype)
    hidden = append(dq)
    image = synthesize(hidden[:, 1:-1, :])
    feats = model.model.clip_vision_embedding(clip_pixels(model, image))
    sp = model.model.embed(torch.as_tensor([[layout.im_start, layout.im_end]], device=dq.device))
    hidden = append(torch.cat([sp[:, :1], feats.to(sp.dtype), sp[:, 1:]], 1))
    logits = ops.linear(hidden[:, -1:], model.lm_head.weight, out_fp32=True)
    return image[0], logits[0, 0].float()


@torch.no_grad()
def interleaved_decode(model, input_ids, max_new_tokens, max_images, temperature, top_k, top_p, images, attention_mask, seed, fast,
                       use_graph, eos, pad, greedy, synthesize):
    """Body of `DreamLLMForCausalMLM.generate_interleaved` (INTEGRATION.md "Interleaved generation").  Token choice as `sampled_decode`
    (`ops.sample_logits` over the whole vocabulary); a row that emits <dream_start> gets [<dream_start>, queries, <dream_end>] and,
    after `synthesize(prompt_embeds [1, n_query, d], row) -> image fp32 [1, 3, H, W] in [0, 1]`, [<im_start>, CLIP patch embeddings,
    <im_end>] appended to its cache and carries on from the logits at <im_end>.

    `fast=False` (and B > 8) is the specification: every row on its own, the model forward re-entered per token and per block with
    `past_key_values`.  The fast path runs `decode.InterleavedDecodeSession`: chunks of up to 16 graph replays, `parked` read between
    chunks; when no row is running, the rows parked on the trigger get their blocks (`append_block`) and the next phase begins."""
    B, S = input_ids.shape
    dev = input_ids.device
    layout = interleave_layout(model)
    V = model.config.vocab_size
    eos = -1 if eos is None else int(eos)
    if fast is None:
        fast = B <= 8
    if attention_mask is not None:
        plen = [int(n) for n in (attention_mask != 0).sum(-1).tolist()]
    else:
        plen = [S] * B
    prompts = [input_ids[b, S - plen[b]:] for b in range(B)]
    cmax = [trigger_room(layout, plen[b], max_new_tokens, model.config.max_position_embeddings) for b in range(B)]
    out_images = [[] for _ in range(B)]

    if not fast:
        im_rows = (input_ids == layout.im_start).sum(-1).tolist() if images is not None else [0] * B
        seqs, poss = [], []
        buf = torch.zeros(B, V, dtype=torch.float32, device=dev)
        uni = torch.zeros(B, dtype=torch.float32, device=dev) if greedy else None
        tok = torch.empty(B, dtype=torch.long, device=dev)
        for b in range(B):
            i0 = int(sum(im_rows[:b]))
            stepper = ModelStepper(model, prompts[b][None], images[i0:i0 + int(im_rows[b])] if im_rows[b] else None, None)

            def append(embeds):
                out = model.model._forward(inputs_embeds=embeds, past_key_values=stepper.past, use_cache=True, return_dict=True)
                stepper.past = out.past_key_values
                return out.last_hidden_state

            logits = stepper.logits[0].float()
            segs, cur, cnt, n_img, phase, step = [], [], 0, 0, 0, 0
            while cnt < max_new_tokens:
                buf[b].copy_(logits)
                if n_img >= max_images or cnt > cmax[b]:
                    buf[b, layout.trigger] = float("-inf")
                ops.sample_logits(buf, temperature, top_k, top_p, vocab_limit=V, seed=phase_seed(seed, phase),
                                  step=step, tok_out=tok, uniforms=uni)
                t = int(tok[b])
                step += 1
                cnt += 1
                cur.append(t)
                if t == eos:
                    break
                if t == layout.trigger:
                    image, logits = _image_event(model, layout, append, lambda e: synthesize(e, b, n_img))
                    out_images[b].append(image)
                    segs.append((cur, True))
                    cur, cnt, n_img, phase, step = [], cnt + layout.block_len, n_img + 1, phase + 1, 0
                elif cnt < max_new_tokens:
                    logits = stepper.step(tok[b:b + 1].clone())[0].float()
            if cur:
                segs.append((cur, False))
            seq, pos = assemble_row(prompts[b], segs, layout)
            seqs.append(seq)
            poss.append(pos)
        return InterleavedOutput(seqs, out_images, poss)

    from .decode import InterleavedDecodeSession
    max_len = S + max_new_tokens + 1
    sess = cached_session(
        model, ("interleave", B, max_len, use_graph, temperature, top_k, top_p, eos, int(pad), greedy, layout.trigger),
        lambda: InterleavedDecodeSession(model, B, max_len, temperature, top_k, top_p, eos=eos, pad=pad, trigger=layout.trigger,
                                         use_graph=use_graph, fixed_u=0.0 if greedy else None, weights=decode_weights(model)))
    cnt, n_img = [0] * B, [0] * B                # new tokens so far (layout included), images so far
    cur, pos = [S] * B, list(plen)               # cache slot and position id of the row's first token of the phase
    start = [S - n for n in plen]
    alive = list(range(B))
    banned = [None] * B

    def ban(b, c_next):
        want = n_img[b] >= max_images or c_next > cmax[b]
        if banned[b] != want:
            sess.set_ban(b, want)
            banned[b] = want

    for b in range(B):
        ban(b, 0)
    sess.prefill(input_ids, images=images, attention_mask=attention_mask, seed=seed)
    phases, phase = [], 0
    while True:
        parts, n_phase = [sess._out_all[:1].clone()], 1
        taken, running = [0] * B, list(alive)
        while True:
            parked, pstep = sess.parked.tolist(), sess.park_step.tolist()  # the host reads of a chunk
            for b in list(running):
                if parked[b]:
                    taken[b] = int(pstep[b])
                    running.remove(b)
                elif cnt[b] + n_phase >= max_new_tokens:
                    taken[b] = n_phase
                    sess.parked[b] = 1
                    parked[b] = 1
                    running.remove(b)
            if not running:
                break
            m = 16
            for b in running:
                c_next = cnt[b] + n_phase
                ban(b, c_next)
                m = min(m, max_new_tokens - c_next)
                if not banned[b]:
                    m = min(m, cmax[b] - c_next + 1)
            parts.append(sess.generate(m).t())
            n_phase += m
        image_rows = [b for b in alive if parked[b] == 2]
        phases.append((torch.cat(parts, 0), taken, [b in image_rows for b in range(B)]))
        for b in alive:
            cnt[b] += taken[b]
        alive = []
        if not image_rows:
            break
        buf = torch.zeros(B, V, dtype=torch.float32, device=dev)
        for b in image_rows:
            state = dict(cur=cur[b] + taken[b] - 1, pos=pos[b] + taken[b] - 1)

            def append(embeds):
                hidden = sess.append_block(b, embeds, start[b], state["cur"], state["pos"])
                state["cur"] += embeds.shape[1]
                state["pos"] += embeds.shape[1]
                return hidden

            image, logits = _image_event(model, layout, append, lambda e: synthesize(e, b, n_img[b]))
            out_images[b].append(image)
            buf[b].copy_(logits)
            cur[b], pos[b], cnt[b], n_img[b] = state["cur"], state["pos"], cnt[b] + layout.block_len, n_img[b] + 1
            if cnt[b] < max_new_tokens:
                alive.append(b)
                sess.set_row(b, cur[b], pos[b], parked=0)
                ban(b, cnt[b])
            else:
                sess.set_row(b, cur[b], pos[b], parked=1)
        if not alive:
            break
        phase += 1
        sess.begin_phase(buf, phase)
    seqs, poss = assemble_interleaved(prompts, phases, layout)
    return InterleavedOutput(seqs, out_images, poss)


# ------------------------------------------------------------------------------------------------------- best-of-N selection
class BestOfNOutput(NamedTuple):
    """`DreamLLMForCausalMLM.best_of_n`: images fp32 [B, 3, H, W] in [0, 1] (the chosen image of every prompt), index int64 [B] (which
    of the n seeds it came from), logits (a list of B fp32 tensors [n, m_b]: `logits_per_image` of prompt b's n images against its m_b
    captions), seeds (the n seeds, in the order of `index`)."""
    images: torch.Tensor
    index: torch.Tensor
    logits: list
    seeds: list


def check_best_of_n(prompt_ids, negative_prompt_ids, clip, caption_ids, captions_per_prompt, n, seeds, caption_attention_mask,
                    guidance_scale):
    """Every argument check of `best_of_n`, on the host, before any device work -> (seeds, captions_per_prompt) as lists of ints."""
    from .clip_model import HipCLIPModel
    if not isinstance(clip, HipCLIPModel):
        raise ValueError(f"best_of_n: `clip` must be a HipCLIPModel, got {type(clip).__name__}")
    if prompt_ids is None or prompt_ids.dim() != 2:
        raise ValueError("best_of_n: prompt_ids must be [batch, seq]")
    B = prompt_ids.shape[0]
    n = int(n)
    if n < 1:
        raise ValueError(f"best_of_n: `n` must be >= 1, got {n}")
    seeds = list(range(42, 42 + n)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != n:
        raise ValueError(f"best_of_n: `seeds` holds {len(seeds)} seeds for n = {n}")
    caps = [int(c) for c in captions_per_prompt]
    if len(caps) != B:
        raise ValueError(f"best_of_n: `captions_per_prompt` holds {len(caps)} entries for {B} prompts")
    if caption_ids is None or caption_ids.dim() != 2:
        raise ValueError("best_of_n: caption_ids must be [captions, seq]")
    if any(c < 1 for c in caps) or sum(caps) != caption_ids.shape[0]:
        raise ValueError(f"best_of_n: `captions_per_prompt` {caps} (every entry >= 1) must sum to the {caption_ids.shape[0]} rows of caption_ids")
    clip._text.check_inputs(caption_ids, caption_attention_mask)
    if guidance_scale > 1.0:
        if negative_prompt_ids is None:
            raise ValueError("best_of_n: `guidance_scale` > 1 (classifier-free guidance) needs `negative_prompt_ids`")
        if negative_prompt_ids.dim() != 2 or negative_prompt_ids.shape[0] not in (1, B):
            raise ValueError("best_of_n: negative_prompt_ids must be [1, seq] or [batch, seq]")
    return seeds, caps

