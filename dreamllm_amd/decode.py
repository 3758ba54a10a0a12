"""KV-cache greedy decoding of DreamLLMForCausalMLM on the HIP decode kernels, one hipGraph replay per token.

Reference loop: omni/eval/language_eval/modeling_dreamllm.py:76-97 with temperature 0 (argmax, :92) over
DreamLLMForCausalMLM.forward (modeling_dreamllm.py:1353) with `use_cache=True`.  The reference re-enters the whole Python model
per token (~15 kernels x 32 layers + host logic); at batch 1 that is launch-bound by an order of magnitude over the weight
stream.  Here the token step is a fixed sequence of launches on static buffers:

    embed[tok] -> 32 x { [RMSNorm + q/k/v GEMV] -> [RoPE(pos on device) + K/V append to the cache at pos] -> decode attention
    over the cache (valid length on device) -> [o GEMV + residual] -> [RMSNorm + gate/up GEMV + SwiGLU] -> [down GEMV + residual] }
    -> [final RMSNorm + lm_head GEMV] (fp32 logits) -> argmax -> pos/len/step += 1      ([..] = one launch; 7 per layer;
    round 4: RoPE + append folded into the attention launch -> 6 per layer)

The two 5-launch forms (the split-KV merge inside the attention launch, or inside the o projection's GEMV) were built and measured
slower than the separate combine launch (DESIGN.md "Decode"; 298.6 against 308.3 tok/s, profiles/r06_decode_merge_ab.log); their
kernels and launchers stay in `ops` with their unit tests, the session no longer exposes them.

The step is captured once per (batch, max_len) in a hipGraph (`torch.cuda.CUDAGraph`) and replayed per token; nothing in it depends
on the host.  Prefill runs through the normal model forward (MFMA GEMMs + flash attention) and its K/V are copied into the cache.

Opt-in FP8 weight-only decoding (`weights=DecodeWeightsFP8.from_model(model)`, `model.quantize_decode_weights`): the four GEMV launches
of a layer read e4m3 copies of the decoder weights (csrc/gemv_w8.hip) -- half the bytes of the stream that bounds the step.  The
prefill, the embedding, the norms and lm_head stay bf16: the prompt is encoded with W, the new tokens with Q(W).
"""
from __future__ import annotations

import math

import torch

from . import ops
from .generation import check_left_padded, left_pad_position_ids, phase_seed


class DecodeWeightsFP8:
    """FP8 (OCP e4m3fn) copies of the decoder's Linear weights for the token step: `ops.quantize_rows_e4m3` of every q/k/v/o and
    gate/up/down projection, one fp32 scale per output row.  `layers[i]` holds `qkv` / `qkv_scale` (the q|k|v rows packed into one
    matrix with one scale vector; `qkv_parts` / `qkv_scale_parts` are the three matrices as views of them) and `o`, `gate`, `up`,
    `down` with their `*_scale`.  The embedding, the norms and `lm_head` are not quantised: a session reads them from the model.

    A plain holder and a SNAPSHOT: it does not follow later changes of the model's weights; build it again after they change."""

    def __init__(self, layers):
        self.layers = layers

    @classmethod
    @torch.no_grad()
    def from_model(cls, model):
        layers = []
        for layer in model.model.layers:
            at, mlp = layer.self_attn, layer.mlp
            qkv = [ops.quantize_rows_e4m3(p.weight.detach()) for p in (at.q_proj, at.k_proj, at.v_proj)]
            rows = [q.shape[0] for q, _ in qkv]
            # packed as bytes: torch.cat has no float8 kernel on every build
            e = {"qkv": torch.cat([q.view(torch.uint8) for q, _ in qkv]).view(torch.float8_e4m3fn),
                 "qkv_scale": torch.cat([s for _, s in qkv])}
            e["qkv_parts"], e["qkv_scale_parts"] = e["qkv"].split(rows), e["qkv_scale"].split(rows)
            for name, lin in (("o", at.o_proj), ("gate", mlp.gate_proj), ("up", mlp.up_proj), ("down", mlp.down_proj)):
                e[name], e[name + "_scale"] = ops.quantize_rows_e4m3(lin.weight.detach())
            layers.append(e)
        return cls(layers)

    def nbytes(self):
        """Device bytes of the codes and scales."""
        return sum(t.numel() * t.element_size() for e in self.layers for t in e.values() if isinstance(t, torch.Tensor))


class GreedyDecodeSession:
    def __init__(self, model, batch_size: int, max_len: int, use_graph: bool = True, nsplit: int = 8, fused: bool = True,
                 vocab_limit: int | None = 32000, weights: DecodeWeightsFP8 | None = None):
        """`vocab_limit`: argmax runs over `logits[..., :vocab_limit]` -- the reference loop slices `[..., :32000]`
        (omni/eval/language_eval/modeling_dreamllm.py:79,86) so that none of the added special tokens (<dream_start>, <im_*>,
        [PAD] ...) can be emitted; None = whole vocabulary.  `fused=False`: the token step one launch per operation, the
        reference form of the fused step in the tests.

        `weights`: a `DecodeWeightsFP8` -- the token step then streams the FP8 copies of the decoder's Linear weights (`ops.gemv_w8`
        / `ops.gemv_fused_w8`, the same launches in the same places, so graph capture is unchanged).  The embedding, the norms and
        `lm_head` stay bf16, and the PREFILL stays on the bf16 model forward: the prompt is encoded with W, the new tokens with
        Q(W)."""
        cfg = model.config
        self.model = model
        self.weights = weights
        self.B, self.max_len, self.use_graph, self.nsplit, self.fused = batch_size, max_len, use_graph, nsplit, fused
        if batch_size > 8:
            raise ValueError("the decode GEMV handles up to 8 sequences per step")
        dev, dt = model.device, model.dtype
        self.H, self.Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
        self.D = cfg.hidden_size // self.H
        L = cfg.num_hidden_layers
        self.kc = [torch.zeros(batch_size, max_len, self.Hkv, self.D, dtype=dt, device=dev) for _ in range(L)]
        self.vc = [torch.zeros(batch_size, max_len, self.Hkv, self.D, dtype=dt, device=dev) for _ in range(L)]
        self.tok = torch.zeros(batch_size, dtype=torch.long, device=dev)          # token fed to the next step
        self.pos = torch.zeros(batch_size, 1, dtype=torch.long, device=dev)       # its position id
        self.kv_len = torch.zeros(batch_size, dtype=torch.int32, device=dev)      # valid cache length INCLUDING that token
        self.slot = torch.zeros(batch_size, dtype=torch.long, device=dev)         # row of cache.view(B*max_len, -1) to write
        self.step_idx = torch.zeros(1, dtype=torch.long, device=dev)
        self.out_tokens = torch.zeros(max_len, batch_size, dtype=torch.long, device=dev)
        self.vocab_limit = cfg.vocab_size if vocab_limit is None else min(int(vocab_limit), cfg.vocab_size)
        self.kv_start = torch.zeros(batch_size, dtype=torch.int32, device=dev)    # first valid cache slot (left-padded prompts)
        # teacher forcing of rows that are still inside their prompt (ragged batches, reference loop :93-94): step i emits
        # force_tok[i] where force_mask[i] is set, the argmax otherwise
        self.force_tok = torch.zeros(max_len, batch_size, dtype=torch.long, device=dev)
        self.force_mask = torch.zeros(max_len, batch_size, dtype=torch.bool, device=dev)
        rope = model.model.layers[0].self_attn.rotary_emb
        self.cos, self.sin = rope.tables(max_len, dev)
        self.row_map = None  # beam search: int32 [B, max_len] copy-free KV map (BeamDecodeSession); None = every row reads itself
        self.graph = None
        self.logits = None

    # ---- one token -------------------------------------------------------------------------------------------------
    def _token_step(self):
        m = self.model
        cfg = m.config
        B, H, Hkv, D = self.B, self.H, self.Hkv, self.D
        eps = cfg.rms_norm_eps
        x = m.model.embed_tokens.weight.index_select(0, self.tok)  # [B, d]
        pos = self.pos.view(-1)
        layers = m.model.layers
        if self.weights is not None:  # FP8 copies of the decoder's Linear weights: the same launches over ops.gemv*_w8
            x, layers = self._layers_w8(x, pos), ()
        for li, layer in enumerate(layers):
            at, mlp = layer.self_attn, layer.mlp
            if self.fused:
                # 6 launches per layer: [RMSNorm + q/k/v GEMV] [RoPE + cache append + attention x2] [o GEMV + residual]
                # [RMSNorm + gate/up GEMV + SwiGLU] [down GEMV + residual]
                q, k, v = ops.gemv_fused(x, (at.q_proj.weight, at.k_proj.weight, at.v_proj.weight),
                                         norm_w=layer.input_layernorm.weight, eps=eps)
                o = ops.attn_decode_rope(q.view(B, H, D), k.view(B, Hkv, D), v.view(B, Hkv, D), self.kc[li], self.vc[li], self.kv_len,
                                         self.cos, self.sin, pos, 1.0 / math.sqrt(D), self.nsplit, kv_start=self.kv_start,
                                         row_map=self.row_map)
                x2 = ops.gemv(o.view(B, H * D), at.o_proj.weight, residual=x)
                act = ops.gemv_fused(x2, (mlp.gate_proj.weight, mlp.up_proj.weight), norm_w=layer.post_attention_layernorm.weight,
                                     eps=eps, swiglu=True)
                x = ops.gemv(act, mlp.down_proj.weight, residual=x2)
                continue
            h, _, _ = ops.rmsnorm_fwd(x, layer.input_layernorm.weight, eps)
            q = ops.gemv(h, at.q_proj.weight).view(B, 1, H, D)
            k = ops.gemv(h, at.k_proj.weight).view(B, 1, Hkv, D)
            v = ops.gemv(h, at.v_proj.weight)
            ops.rope_(q, self.cos, self.sin, self.pos)
            ops.rope_(k, self.cos, self.sin, self.pos)
            self.kc[li].view(B * self.max_len, Hkv * D).index_copy_(0, self.slot, k.view(B, Hkv * D))
            self.vc[li].view(B * self.max_len, Hkv * D).index_copy_(0, self.slot, v)
            o = ops.attn_decode(q.view(B, H, D), self.kc[li], self.vc[li], self.kv_len, 1.0 / math.sqrt(D), self.nsplit,
                                kv_start=self.kv_start, row_map=self.row_map)
            x2 = ops.gemv(o.view(B, H * D), at.o_proj.weight, residual=x)
            h2, _, _ = ops.rmsnorm_fwd(x2, layer.post_attention_layernorm.weight, eps)
            g = ops.gemv(h2, mlp.gate_proj.weight)
            u = ops.gemv(h2, mlp.up_proj.weight)
            x = ops.gemv(ops.glu_fwd(g, u, 0), mlp.down_proj.weight, residual=x2)
        if self.fused:
            logits = ops.gemv_fused(x, (m.lm_head.weight,), norm_w=m.model.norm.weight, eps=eps, out_dtype=torch.float32)[0]
        else:
            hf, _, _ = ops.rmsnorm_fwd(x, m.model.norm.weight, eps)
            logits = ops.gemv(hf, m.lm_head.weight, out_dtype=torch.float32)
        self._choose(logits)
        self._advance()
        return logits

    def _layers_w8(self, x, pos):
        """The decoder layers of `_token_step` over `self.weights` (FP8 codes + per-row scales): launch for launch the bf16 loop, in
        the fused and in the one-launch-per-operation form."""
        B, H, Hkv, D = self.B, self.H, self.Hkv, self.D
        eps = self.model.config.rms_norm_eps
        scale = 1.0 / math.sqrt(D)
        for li, (layer, w) in enumerate(zip(self.model.model.layers, self.weights.layers)):
            qkv, qs = w["qkv_parts"], w["qkv_scale_parts"]
            if self.fused:
                q, k, v = ops.gemv_fused_w8(x, qkv, qs, norm_w=layer.input_layernorm.weight, eps=eps)
                o = ops.attn_decode_rope(q.view(B, H, D), k.view(B, Hkv, D), v.view(B, Hkv, D), self.kc[li], self.vc[li], self.kv_len,
                                         self.cos, self.sin, pos, scale, self.nsplit, kv_start=self.kv_start, row_map=self.row_map)
                x2 = ops.gemv_w8(o.view(B, H * D), w["o"], w["o_scale"], residual=x)
                act = ops.gemv_fused_w8(x2, (w["gate"], w["up"]), (w["gate_scale"], w["up_scale"]),
                                        norm_w=layer.post_attention_layernorm.weight, eps=eps, swiglu=True)
                x = ops.gemv_w8(act, w["down"], w["down_scale"], residual=x2)
                continue
            h, _, _ = ops.rmsnorm_fwd(x, layer.input_layernorm.weight, eps)
            q = ops.gemv_w8(h, qkv[0], qs[0]).view(B, 1, H, D)
            k = ops.gemv_w8(h, qkv[1], qs[1]).view(B, 1, Hkv, D)
            v = ops.gemv_w8(h, qkv[2], qs[2])
            ops.rope_(q, self.cos, self.sin, self.pos)
            ops.rope_(k, self.cos, self.sin, self.pos)
            self.kc[li].view(B * self.max_len, Hkv * D).index_copy_(0, self.slot, k.view(B, Hkv * D))
            self.vc[li].view(B * self.max_len, Hkv * D).index_copy_(0, self.slot, v)
            o = ops.attn_decode(q.view(B, H, D), self.kc[li], self.vc[li], self.kv_len, scale, self.nsplit,
                                kv_start=self.kv_start, row_map=self.row_map)
            x2 = ops.gemv_w8(o.view(B, H * D), w["o"], w["o_scale"], residual=x)
            h2, _, _ = ops.rmsnorm_fwd(x2, layer.post_attention_layernorm.weight, eps)
            g = ops.gemv_w8(h2, w["gate"], w["gate_scale"])
            u = ops.gemv_w8(h2, w["up"], w["up_scale"])
            x = ops.gemv_w8(ops.glu_fwd(g, u, 0), w["down"], w["down_scale"], residual=x2)
        return x

    def _advance(self):
        """End of a token step (inside the captured graph): every row moves on to its next position and cache slot."""
        self.pos.add_(1)
        self.kv_len.add_(1)
        self.slot.add_(1)

    def _choose(self, logits):
        """Token choice of a step (inside the captured graph): writes `tok` and `out_tokens[step]`, advances the step."""
        nxt = logits[:, : self.vocab_limit].argmax(-1)
        nxt = torch.where(self.force_mask.index_select(0, self.step_idx)[0], self.force_tok.index_select(0, self.step_idx)[0], nxt)
        self.out_tokens.index_copy_(0, self.step_idx, nxt[None])
        self.tok.copy_(nxt)
        self.step_idx.add_(1)

    def _choose_first(self, logits, forced_tok, forced_mask):
        """First token after the prompt from the prefill's last-position logits [B, V]; forced_tok / forced_mask [B] or None."""
        first = logits[:, : self.vocab_limit].argmax(-1)
        if forced_tok is not None:
            first = torch.where(forced_mask, forced_tok, first)
        return first

    def _state(self):
        """Device state a token step changes (saved around the warm-up step before capture)."""
        return (self.tok, self.pos, self.kv_len, self.slot, self.step_idx, self.out_tokens)

    def _prefill_prompt(self, input_ids, images, attention_mask, rows=1):
        """Prompt [B, S] through the model (MFMA path), its K/V into cache rows b * rows, and the step state of all B * rows session
        rows set for the first token step.  -> last-position logits [B, V]; the caller chooses the first token from them.

        `attention_mask` (LEFT padding, the layout of the reference's batched generate() callers,
        omni/eval/vqa/vqa_inference.py:276): position ids are mask-aware as HF generate computes them; every row's next token goes
        to cache slot S, its position is the row's own length, and the pad slots in front are masked in the token steps
        (`kv_start`).  Right-padded or holey masks raise (`check_left_padded`)."""
        B, S = input_ids.shape
        if B * rows != self.B or S >= self.max_len:
            raise ValueError(f"prompt [{B},{S}] does not fit the session (batch {self.B // rows}, max_len {self.max_len})")
        dev = self.tok.device
        position_ids = None

        def per_row(t):  # [B] -> [B * rows]
            return t.repeat_interleave(rows) if rows > 1 else t

        if attention_mask is not None:
            am = attention_mask.to(dev) != 0
            start, lens = check_left_padded(am, type(self).__name__ + ".prefill")
            position_ids = left_pad_position_ids(am)
            self.kv_start.copy_(per_row(start.to(torch.int32)))
            self.pos.copy_(per_row(lens)[:, None])
        else:
            self.kv_start.zero_()
            self.pos.fill_(S)
        out = self.model(input_ids=input_ids, images=images, attention_mask=attention_mask, position_ids=position_ids,
                         use_cache=True, return_dict=True)
        for li, (k, v) in enumerate(out.past_key_values):  # reference layout [B, Hkv, S, D]
            self.kc[li][::rows, :S].copy_(k.transpose(1, 2))
            self.vc[li][::rows, :S].copy_(v.transpose(1, 2))
        self.kv_len.fill_(S + 1)
        self.slot.copy_(torch.arange(self.B, device=dev) * self.max_len + S)
        self.step_idx.zero_()
        self.prompt_len = S
        self.generated = 0  # tokens produced by generate() since this prefill (host-side count of graph replays)
        return out.logits[:, -1]

    # ---- public ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill(self, input_ids, images=None, attention_mask=None, forced_tokens=None, forced_mask=None):
        """Run the prompt through the model, fill the cache (`_prefill_prompt`), emit the first new token.

        `forced_tokens` / `forced_mask` [B, n]: token i after the prompt is forced to `forced_tokens[:, i]` where
        `forced_mask[:, i]` is set (teacher forcing of rows still inside their prompt, reference loop :93-94)."""
        logits = self._prefill_prompt(input_ids, images, attention_mask)
        dev = self.tok.device
        self.force_mask.zero_()
        f_tok = f_mask = None
        if forced_tokens is not None:
            n = forced_tokens.shape[1]
            if n > 0:
                f_tok, f_mask = forced_tokens[:, 0].to(dev), forced_mask[:, 0].to(dev)
                self.force_tok[: n - 1].copy_(forced_tokens[:, 1:].t())
                self.force_mask[: n - 1].copy_(forced_mask[:, 1:].t())
        first = self._choose_first(logits, f_tok, f_mask)
        self.tok.copy_(first)
        return first

    @torch.no_grad()
    def generate(self, n_more: int):
        """n_more further tokens after those already produced since `prefill`; returns [B, n_more] (may be called repeatedly)."""
        if self.prompt_len + 1 + self.generated + n_more > self.max_len:
            raise ValueError("generation would overflow the KV cache")
        if n_more <= 0:
            return self.out_tokens[:0].t()
        if self.use_graph and self.graph is None:
            state = [t.clone() for t in self._state()]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up outside capture
                self._token_step()
            torch.cuda.current_stream().wait_stream(side)
            for t, s in zip(self._state(), state):
                t.copy_(s)  # the warm-up wrote cache row `slot`, which the first real step rewrites identically
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.logits = self._token_step()
            for t, s in zip(self._state(), state):
                t.copy_(s)  # capture does not execute, but keep the state explicit
        for _ in range(n_more):
            if self.use_graph:
                self.graph.replay()
            else:
                self.logits = self._token_step()
        start = self.generated
        self.generated += n_more
        return self.out_tokens[start:start + n_more].t().contiguous()


class SampledDecodeSession(GreedyDecodeSession):
    """`GreedyDecodeSession` whose token choice samples (`ops.sample_logits`, csrc/sample.hip): temperature, top-k, top-p, the draw,
    teacher forcing, HF's finished-row rule and the step counter in ONE launch inside the captured graph, in place of the greedy
    step's argmax + bookkeeping launches.

    u comes from Philox4x32-10 keyed by the seed given to `prefill` (a device buffer) at counter (row, step): the prefill's token is
    step 0 and graph replay i is step i + 1.  With `eos` >= 0 a row that has emitted eos emits `pad` from then on (`finished`, a
    device buffer, reset by `prefill`)."""

    def __init__(self, model, batch_size: int, max_len: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                 eos: int | None = None, pad: int = 0, fixed_u: float | None = None, **kw):
        super().__init__(model, batch_size, max_len, **kw)
        if not temperature > 0:
            raise ValueError("SampledDecodeSession: temperature must be > 0 (use GreedyDecodeSession for temperature 0)")
        if self.vocab_limit > 32768:
            raise ValueError("SampledDecodeSession: the sampling kernel covers at most 32768 ids")
        dev = self.tok.device
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.eos, self.pad = (-1 if eos is None else int(eos)), int(pad)
        # the kernel indexes [step][b] with step 0 = the prefill's token: row 0 of these buffers belongs to it, rows 1.. are the
        # greedy session's out_tokens / force_tok / force_mask (views, so the inherited prefill / generate index them unchanged)
        self._out_all = torch.zeros(max_len + 1, batch_size, dtype=torch.long, device=dev)
        self._ftok_all = torch.zeros(max_len + 1, batch_size, dtype=torch.long, device=dev)
        self._fmask_all = torch.zeros(max_len + 1, batch_size, dtype=torch.bool, device=dev)
        self.out_tokens, self.force_tok, self.force_mask = self._out_all[1:], self._ftok_all[1:], self._fmask_all[1:]
        self.seed = torch.zeros(1, dtype=torch.long, device=dev)
        self.rng_step = torch.zeros(1, dtype=torch.long, device=dev)
        self.arrive = torch.zeros(1, dtype=torch.int32, device=dev)
        self.finished = torch.zeros(batch_size, dtype=torch.bool, device=dev)
        self.status = torch.zeros(batch_size, dtype=torch.int32, device=dev)
        # fixed_u: every draw uses this u instead of the Philox stream (0 with top-k 1 = greedy search)
        self.uniforms = None if fixed_u is None else torch.full((batch_size,), float(fixed_u), dtype=torch.float32, device=dev)

    def _sample(self, logits):
        ops.sample_logits(logits, self.temperature, self.top_k, self.top_p, vocab_limit=self.vocab_limit, seed=self.seed,
                          step=self.rng_step, out_tokens=self._out_all, force_tok=self._ftok_all, force_mask=self._fmask_all,
                          eos=self.eos, pad=self.pad, finished=self.finished, tok_out=self.tok, status=self.status,
                          advance_step=True, arrive=self.arrive, uniforms=self.uniforms)

    def _choose(self, logits):
        self._sample(logits)

    def _choose_first(self, logits, forced_tok, forced_mask):
        if forced_tok is not None:
            self._ftok_all[0].copy_(forced_tok)
            self._fmask_all[0].copy_(forced_mask)
        else:
            self._fmask_all[0].zero_()
        self.rng_step.zero_()
        self.finished.zero_()
        self.status.zero_()
        self.first_logits = logits.float()
        self._sample(self.first_logits)
        return self._out_all[0].clone()

    def _state(self):
        return super()._state() + (self.rng_step, self.finished, self.status)

    @torch.no_grad()
    def prefill(self, input_ids, images=None, attention_mask=None, forced_tokens=None, forced_mask=None, seed: int = 0):
        """`GreedyDecodeSession.prefill` with the first token sampled; `seed` (int64) keys every draw until the next prefill."""
        self.seed.fill_(int(seed))
        return super().prefill(input_ids, images=images, attention_mask=attention_mask, forced_tokens=forced_tokens,
                               forced_mask=forced_mask)


class BeamDecodeSession(GreedyDecodeSession):
    """Beam search on the decode kernels: a `GreedyDecodeSession` over B * nb rows (row r = b * nb + beam) whose token choice is
    `ops.beam_step` (csrc/beam.hip, one launch inside the captured graph) and whose attention reads the cache through a row map.

    The KV cache is never copied or reordered: each row writes its own token to its own slot, and `row_map[r, j]` names the row
    whose cache holds slot j of beam r's history.  The beam step permutes the map (map[r, :c + 1] = map[parent(r), :c + 1],
    map[r, c + 1] = r); entries only ever point at older slots, which nobody writes again.  The prompt is prefilled once per batch
    into row b * nb, and every beam's map points there.  Step 0 (from the prefill's logits) is HF's step 0: the beams with score
    -1e9 cannot be chosen, so it runs the same kernel on the prompt logits repeated nb times."""

    def __init__(self, model, batch_size: int, num_beams: int, max_len: int, eos: int | None = None, pad: int = 0,
                 length_penalty: float = 1.0, early_stopping=False, max_new: int = 0, **kw):
        if batch_size * num_beams > 8:
            raise ValueError("BeamDecodeSession: the decode GEMV handles up to 8 rows (batch * num_beams) per step")
        super().__init__(model, batch_size * num_beams, max_len, vocab_limit=None, **kw)
        dev = self.tok.device
        self.nbatch, self.nb = batch_size, num_beams
        self.eos, self.pad = (-1 if eos is None else int(eos)), int(pad)
        self.length_penalty, self.early_stopping, self.max_new = float(length_penalty), early_stopping, int(max_new)
        self.beam = ops.BeamState(batch_size, num_beams, max_len + 1, dev)
        self.tok = self.beam.tok  # the beam step writes the next tokens where the token step reads them
        self.row_map = torch.zeros(self.B, max_len, dtype=torch.int32, device=dev)

    def _choose(self, logits):
        ops.beam_step(logits, self.beam, eos=self.eos, pad=self.pad, length_penalty=self.length_penalty,
                      early_stopping=self.early_stopping, max_new=self.max_new, kv_len=self.kv_len, row_map=self.row_map)

    def _state(self):
        return super()._state() + self.beam.tensors() + (self.row_map,)

    @torch.no_grad()
    def prefill(self, input_ids, images=None, attention_mask=None):
        """Prompt [B, S] (LEFT-padded with `attention_mask`) through the model once per batch; its K/V go to row b * nb, every beam's
        map points there; then beam step 0 from the last-position logits.  Returns the step's tokens [B * nb]."""
        nb, R = self.nb, self.B
        logits = self._prefill_prompt(input_ids, images, attention_mask, rows=nb)
        rows = torch.arange(R, device=self.tok.device, dtype=torch.int32)
        self.row_map.copy_((rows // nb * nb)[:, None].expand(R, self.max_len))
        self.row_map[:, self.prompt_len] = rows
        self.beam.reset()
        self.beam.status.zero_()
        self.first_logits = logits.float().repeat_interleave(nb, 0)
        ops.beam_step(self.first_logits, self.beam, eos=self.eos, pad=self.pad, length_penalty=self.length_penalty,
                      early_stopping=self.early_stopping, max_new=self.max_new)
        return self.tok.clone()


class InterleavedDecodeSession(SampledDecodeSession):
    """`SampledDecodeSession` for interleaved text-and-image generation (`generation.interleaved_decode`, INTEGRATION.md "Interleaved
    generation"): rows stop on their own inside a chunk of graph replays, and the host appends whole blocks of embeddings to a row.

    * The end of the token step is `ops.interleave_park` (csrc/interleave.hip) in place of the three unconditional increments: a row
      that has just emitted eos or `trigger` (<dream_start>) is parked (`parked` int32 [B]: 0 running, 1 eos, 2 trigger; `park_step`
      = the number of tokens of the phase up to and including that one) and stops advancing; it keeps re-running its step on one
      dead cache slot, and the host ignores what it emits.
    * `bias` fp32 [B, V] is added to the logits before the token choice (zero, or -inf at the trigger id for a row whose image budget
      or space is used up); the captured graph reads its current values.
    * A PHASE is the stretch between two points at which every row is parked.  Its first token is chosen from given logits
      (`prefill`: the prompt's; `begin_phase`: the logits at <im_end> of the rows that resume), its draws are keyed by
      `generation.phase_seed(seed, phase)` at counter (row, token index within the phase).  A row alive in phase p has produced
      exactly p images, so a row's draws depend on its row index and its own history, not on the other rows of the batch.
    * `append_block(b, embeds)`: one forward of a block of embeddings on the MFMA path against the row's past K/V, taken as views of
      the session cache, with the new K/V written back at the row's own slots."""

    def __init__(self, model, batch_size: int, max_len: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                 eos: int | None = None, pad: int = 0, trigger: int = -1, fixed_u: float | None = None, **kw):
        super().__init__(model, batch_size, max_len, temperature, top_k, top_p, eos=eos, pad=pad, fixed_u=fixed_u, vocab_limit=None, **kw)
        dev = self.tok.device
        self.trigger = int(trigger)
        self.parked = torch.zeros(batch_size, dtype=torch.int32, device=dev)
        self.park_step = torch.zeros(batch_size, dtype=torch.long, device=dev)
        self.bias = torch.zeros(batch_size, model.config.vocab_size, dtype=torch.float32, device=dev)
        self.base_seed = 0

    def _choose(self, logits):
        logits.add_(self.bias)
        self._sample(logits)

    def _advance(self):
        ops.interleave_park(self.tok, self.parked, self.park_step, self.rng_step, eos=self.eos, trigger=self.trigger,
                            pos=self.pos.view(-1), kv_len=self.kv_len, slot=self.slot)

    def _state(self):
        return super()._state() + (self.parked, self.park_step)

    def _choose_first(self, logits, forced_tok, forced_mask):
        self.parked.zero_()
        self.park_step.zero_()
        return self.begin_phase(logits.float(), 0)

    @torch.no_grad()
    def prefill(self, input_ids, images=None, attention_mask=None, seed: int = 0):
        """Prompt through the model, cache filled, phase 0 begun: returns its first token [B] (a row may be parked by it already)."""
        self.base_seed = int(seed)
        return super().prefill(input_ids, images=images, attention_mask=attention_mask, seed=seed)

    @torch.no_grad()
    def begin_phase(self, logits, phase: int):
        """First token of phase `phase` from `logits` fp32 [B, V] (rows that stay parked: any finite values, their token is ignored):
        restarts the step counter, keys the phase's draws, chooses and parks without advancing -- the rows' state already describes
        the slot and position of this token."""
        self.seed.fill_(phase_seed(self.base_seed, phase))
        self._fmask_all[0].zero_()
        self.rng_step.zero_()
        self.status.zero_()
        self.finished.copy_(self.parked != 0)
        self.generated = 0
        self.first_logits = logits + self.bias
        self._sample(self.first_logits)
        ops.interleave_park(self.tok, self.parked, self.park_step, self.rng_step, eos=self.eos, trigger=self.trigger)
        return self._out_all[0].clone()

    def set_ban(self, b: int, banned: bool):
        """Remove (or allow again) the trigger id from row b's token choice."""
        if self.trigger >= 0:
            self.bias[b, self.trigger] = float("-inf") if banned else 0.0

    def set_row(self, b: int, cur: int, pos: int, parked: int = 0):
        """Host-side reset of row b: its next token goes to cache slot `cur` of the row with position id `pos`."""
        self.pos[b, 0] = pos
        self.kv_len[b] = cur + 1
        self.slot[b] = b * self.max_len + cur
        self.parked[b] = parked

    @torch.no_grad()
    def append_block(self, b: int, embeds, start: int, cur: int, pos: int):
        """Run `embeds` [1, L, d] as the next L positions of row b: its valid cache is slots [start, cur), the block takes position
        ids pos .. pos + L - 1 and its K/V go to slots [cur, cur + L).  -> the block's last hidden states [1, L, d]."""
        L = embeds.shape[1]
        if cur + L > self.max_len:
            raise ValueError("append_block: the block does not fit the KV cache")
        past = tuple((k[b:b + 1, start:cur].transpose(1, 2), v[b:b + 1, start:cur].transpose(1, 2)) for k, v in zip(self.kc, self.vc))
        position_ids = torch.arange(pos, pos + L, dtype=torch.long, device=embeds.device)[None]
        out = self.model.model._forward(inputs_embeds=embeds, position_ids=position_ids, past_key_values=past, use_cache=True,
                                        return_dict=True)
        for li, (k, v) in enumerate(out.past_key_values):  # reference layout [1, Hkv, past + L, D]
            self.kc[li][b, cur:cur + L].copy_(k[0, :, -L:].transpose(0, 1))
            self.vc[li][b, cur:cur + L].copy_(v[0, :, -L:].transpose(0, 1))
        return out.last_hidden_state
