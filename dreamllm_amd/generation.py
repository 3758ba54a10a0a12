"""Host side of text generation for `DreamLLMForCausalMLM`: the protocols of the reference's generation loops, each written once.

`greedy_generate`, `sample_generate` and `generate` on the model are argument handling plus one call of a driver here
(`greedy_decode`, `sampled_decode`, `beam_decode`).  A driver either runs a `decode` session (fast path: one hipGraph replay per
token, the host only reads flags between chunks of replays -- `run_chunked`) or re-enters the model forward per token like the
reference (`ModelStepper`).  The drivers differ in how a token is chosen (arg-max / `ops.sample_logits` / `ops.beam_step`);
position ids, the ragged-prompt protocol, the stopping-criterion rule and the session cache are shared.  Everything above the
drivers is index arithmetic on whatever device its arguments live on, so it runs (and is tested) without a GPU.
"""
from __future__ import annotations

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


def cached_session(model, key, factory):
    """The model's one decode session (`model._decode_session = (key, session)`, assignable to None to drop it): equal calls reuse
    it and its captured graph, a call of another kind or shape replaces it.  `key`: a tuple starting with the session kind."""
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
                              lambda: GreedyDecodeSession(model, B, max_len, use_graph=use_graph, vocab_limit=V))
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
                                         vocab_limit=V, fixed_u=0.0 if greedy else None))
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
                                      early_stopping=early_stopping, max_new=max_new_tokens, use_graph=use_graph))
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
