"""Full CLIP (text tower + vision tower + projection heads + similarity) on HIP kernels, forward only -- replaces the
`transformers.CLIPModel` of omni/eval/text2img/ddp_sample_coco.py `select_image`, which scores the eight images sampled for a
caption set and keeps the one that owns the largest entry of `logits_per_image`.

state_dict keys are exactly those of `transformers.CLIPModel` (`text_model.embeddings.{token,position}_embedding.weight`,
`text_model.encoder.layers.{i}.*`, `text_model.final_layer_norm.*`, `vision_model.*` as in clip_vit.py, `visual_projection.weight`,
`text_projection.weight`, `logit_scale`), so `load_state_dict(hf_model.state_dict(), strict=True)` works; the `position_ids`
buffers older checkpoints carry are ignored.

Execution.  Text tower: token rows gathered + position table added, then per layer the vision tower's layer with the causal
bit set: LN -> packed QKV GEMM (+bias) -> causal flash attention with `seqlens` -> out-proj GEMM with bias + residual -> LN -> fc1
GEMM with bias + activation epilogue -> fc2 GEMM with bias + residual.  `final_layer_norm` is NOT run over the sequence: only the
pooled row needs it, and `ops.clip_embed_head` (csrc/clip_score.hip) does pooled row -> LayerNorm -> projection -> L2 normalise
in one launch, for either tower (the vision side pools row 0 through `post_layernorm` and `visual_projection`).  Similarities
and the selection are one `ops.clip_select` launch.  INTEGRATION.md "Best-of-N selection" has the rules.
"""
from __future__ import annotations

import collections
import json
import os
from types import SimpleNamespace

import torch
from torch import nn

from . import ops
from .clip_vit import HipCLIPVisionModel, _Cfg, _Encoder, load_clip_config
from .utils import logger

CLIP_TEXT_L14 = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                     max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu", eos_token_id=2)
CLIP_IMAGE_MEAN = [0.48145466, 0.4578275, 0.40821073]   # CLIPImageProcessor's defaults (OPENAI_CLIP_MEAN / _STD)
CLIP_IMAGE_STD = [0.26862954, 0.26130258, 0.27577711]

ClipSelection = collections.namedtuple("ClipSelection", "best best_logit logits")
ClipSelection.__doc__ = """best int64 [G] (index within its group of the image that owns the largest logit: `argmax(logits_per_image) //
logits_per_image.shape[1]`), best_logit fp32 [G], logits: a list of G fp32 tensors [n_g, m_g] (`logits_per_image` of each group)."""


def _get(c, k, default=None):
    return c.get(k, default) if isinstance(c, dict) else getattr(c, k, default)


def load_clip_text_config(c):
    """A dict or an object with attributes (e.g. `transformers.CLIPTextConfig`) -> the text tower's config; missing entries take
    the CLIP-L/14 values."""
    d = dict(CLIP_TEXT_L14)
    for k in CLIP_TEXT_L14:
        v = _get(c, k)
        if v is not None:
            d[k] = v
    if d["hidden_act"] not in ("quick_gelu", "gelu"):
        raise ValueError(f"CLIP text tower: hidden_act {d['hidden_act']!r} is not supported (quick_gelu or gelu)")
    if d["hidden_size"] % d["num_attention_heads"] or d["hidden_size"] // d["num_attention_heads"] not in (64, 128):
        raise ValueError(f"CLIP text tower: head_dim must be 64 or 128, got {d['hidden_size']} / {d['num_attention_heads']}")
    return _Cfg(**d)


def load_clip_model_config(c):
    """A local HF folder (config.json), a dict, or an object (`transformers.CLIPConfig`) with `text_config`, `vision_config`,
    `projection_dim` and `logit_scale_init_value` -> (text config, vision config, projection_dim, logit_scale_init_value)."""
    if isinstance(c, str):
        fp = os.path.join(c, "config.json")
        if not os.path.isfile(fp):
            raise ValueError(f"HipCLIPModel: {c!r} is not a local directory with a config.json (nothing is downloaded)")
        with open(fp) as f:
            c = json.load(f)
    text, vision = _get(c, "text_config") or {}, _get(c, "vision_config") or {}
    proj = _get(c, "projection_dim")
    return (load_clip_text_config(text), load_clip_config(vision),
            int(768 if proj is None else proj), float(_get(c, "logit_scale_init_value") or 2.6592))


class _TextEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)


class _TextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _TextEmbeddings(cfg)
        self.encoder = _Encoder(cfg)   # the vision tower's layer modules: same parameter names
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


def check_right_padded(attention_mask, shape, who="HipCLIPTextModel"):
    """[B, S] mask of one leading run of ones per row (right padding) -> lengths int32 [B] on the mask's device; anything else
    raises ValueError.  (The check reads the mask on the host.)"""
    if attention_mask.dim() != 2 or tuple(attention_mask.shape) != tuple(shape):
        raise ValueError(f"{who}: attention_mask must have the shape of input_ids {tuple(shape)}, got {tuple(attention_mask.shape)}")
    m = attention_mask != 0
    lens = m.sum(-1)
    run = torch.arange(m.shape[1], device=m.device)[None, :] < lens[:, None]
    if not bool((m == run).all()) or not bool((lens >= 1).all()):
        raise ValueError(f"{who}: attention_mask must be right-padded: one leading run of ones per row (at least one token)")
    return lens.to(torch.int32)


class HipCLIPTextModel(nn.Module):
    """The text tower up to the last encoder layer (`encode`), and its pooled position (`pooled_position`)."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg if isinstance(cfg, _Cfg) else load_clip_text_config(cfg)
        self.text_model = _TextTransformer(self.config)
        self._fused = None  # packed QKV weights (frozen tower), keyed like HipCLIPVisionModel's

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    def _prepare(self):
        ts = []
        for l in self.text_model.encoder.layers:
            a = l.self_attn
            ts += [a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]
        key = (self.device, self.dtype, tuple((t.data_ptr(), t._version) for t in ts))
        if self._fused is not None and self._fused["key"] == key:
            return self._fused
        layers = []
        for l in self.text_model.encoder.layers:
            a = l.self_attn
            layers.append(dict(
                wqkv=torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach().contiguous(),
                bqkv=torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0).detach().contiguous()))
        self._fused = dict(key=key, layers=layers)
        return self._fused

    def check_inputs(self, input_ids, attention_mask=None):
        """Shape checks (host only, before any device work) -> seqlens int32 [B] on the mask's device, or None."""
        if input_ids is None or input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32):
            raise ValueError("HipCLIPTextModel: input_ids must be an integer tensor [batch, seq]")
        S = input_ids.shape[1]
        if not 1 <= S <= self.config.max_position_embeddings:
            raise ValueError(f"HipCLIPTextModel: sequence length {S} outside 1..max_position_embeddings = {self.config.max_position_embeddings}")
        return None if attention_mask is None else check_right_padded(attention_mask, input_ids.shape)

    def pooled_position(self, input_ids):
        """transformers 4.35 `CLIPTextTransformer`: `input_ids.argmax(-1)` when `config.eos_token_id == 2` (the legacy configs, whose
        end-of-text id is the largest in the vocabulary), otherwise the first position holding `eos_token_id`.  On the ids' device,
        nothing is read back."""
        eos = self.config.eos_token_id
        if eos == 2:
            return input_ids.argmax(-1)
        return (input_ids == eos).to(torch.int32).argmax(-1)

    @torch.no_grad()
    def encode(self, input_ids, seqlens=None):
        """-> the last encoder layer's hidden states [B, S, H] (bf16), BEFORE `final_layer_norm`.  `seqlens` int32 [B] on the device:
        the valid tokens of each right-padded row (rows behind them come back as whatever the padding computes: under the causal mask
        no valid row sees them)."""
        cfg, tm = self.config, self.text_model
        f = self._prepare()
        B, S = input_ids.shape
        H, heads = cfg.hidden_size, cfg.num_attention_heads
        D = H // heads
        ids = input_ids.long().clamp(0, cfg.vocab_size - 1)   # device data: a bad id reads a table row, never past the table
        x = ops.gather_rows(tm.embeddings.token_embedding.weight, ids).view(B, S, H)
        x = ops.add_bcast(x, tm.embeddings.position_embedding.weight[:S])
        for l, lf in zip(tm.encoder.layers, f["layers"]):
            h, _, _ = ops.layernorm_fwd(x, l.layer_norm1.weight, l.layer_norm1.bias, cfg.layer_norm_eps, save_stats=False)
            qkv = ops.linear_fwd(h, lf["wqkv"], bias=lf["bqkv"]).view(B, S, 3, heads, D)
            o, _ = ops.attn_fwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], True, D ** -0.5, seqlens=seqlens, need_lse=False)
            x = ops.linear_fwd(o.view(B, S, H), l.self_attn.out_proj.weight, bias=l.self_attn.out_proj.bias, residual=x)
            h, _, _ = ops.layernorm_fwd(x, l.layer_norm2.weight, l.layer_norm2.bias, cfg.layer_norm_eps, save_stats=False)
            h = ops.linear_fwd(h, l.mlp.fc1.weight, bias=l.mlp.fc1.bias, epi=cfg.hidden_act)
            x = ops.linear_fwd(h, l.mlp.fc2.weight, bias=l.mlp.fc2.bias, residual=x)
        return x

    def forward(self, input_ids, attention_mask=None):
        seqlens = self.check_inputs(input_ids, attention_mask)
        ops._need_gpu(input_ids)
        hs = self.encode(input_ids, None if seqlens is None else seqlens.to(input_ids.device))
        return SimpleNamespace(last_hidden_state=hs, pooled_position=self.pooled_position(input_ids))


class HipCLIPModel(nn.Module):
    """`transformers.CLIPModel` for inference: `get_text_features`, `get_image_features`, `forward` (logits_per_image) and
    `select` (the best image of each group of images scored against its group of captions)."""

    def __init__(self, config="openai/clip-vit-large-patch14"):
        super().__init__()
        if isinstance(config, str) and not os.path.isdir(config):
            config = {}   # a preset name: the CLIP-L/14 architecture with random weights (nothing is downloaded)
        tcfg, vcfg, proj, scale0 = load_clip_model_config(config)
        self.config = SimpleNamespace(text_config=tcfg, vision_config=vcfg, projection_dim=proj, logit_scale_init_value=scale0)
        text, vision = HipCLIPTextModel(tcfg), HipCLIPVisionModel(vcfg)
        # the towers' transformer modules are registered HERE under transformers' names; the tower objects that drive them (and cache
        # their packed QKV weights) hold the same modules and stay out of the module tree, so that no key appears twice
        self.text_model = text.text_model
        self.vision_model = vision.vision_model
        self.visual_projection = nn.Linear(vcfg.hidden_size, proj, bias=False)
        self.text_projection = nn.Linear(tcfg.hidden_size, proj, bias=False)
        self.logit_scale = nn.Parameter(torch.tensor(scale0, dtype=torch.float32), requires_grad=False)
        self.__dict__["_text"], self.__dict__["_vision"] = text, vision
        self._scale = None
        self.requires_grad_(False)

    @property
    def device(self):
        return self.text_projection.weight.device

    @property
    def dtype(self):
        return self.text_projection.weight.dtype

    @property
    def image_size(self):
        return self.config.vision_config.image_size

    image_mean, image_std = CLIP_IMAGE_MEAN, CLIP_IMAGE_STD

    def _apply(self, fn, *args, **kwargs):
        # `logit_scale` stays fp32 whatever the towers are cast to: ln(100) rounded to bf16 is a 1 % change of every logit
        keep = self.logit_scale.data.float().clone()
        super()._apply(fn, *args, **kwargs)
        if self.logit_scale.dtype != torch.float32:
            self.logit_scale.data = keep.to(self.logit_scale.device)
        return self

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {k: v for k, v in state_dict.items() if not k.endswith("position_ids")}
        return super().load_state_dict(sd, strict=strict, **kw)

    @classmethod
    def from_pretrained(cls, path, device=None, dtype=torch.bfloat16):
        """A LOCAL directory with config.json and pytorch_model.bin or model.safetensors (as `HipCLIPVisionModel.load_pretrained`:
        nothing is downloaded)."""
        if not isinstance(path, str) or not os.path.isdir(path):
            raise ValueError(f"HipCLIPModel.from_pretrained: {path!r} is not a local directory")
        model = cls(path)
        for fn in ("pytorch_model.bin", "model.safetensors"):
            fp = os.path.join(path, fn)
            if os.path.isfile(fp):
                if fn.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(fp)
                else:
                    sd = torch.load(fp, map_location="cpu")
                model.load_state_dict(sd, strict=True)
                logger.info(f"loaded CLIP weights from {fp}")
                return model.to(device=device, dtype=dtype)
        raise ValueError(f"HipCLIPModel.from_pretrained: no pytorch_model.bin or model.safetensors in {path!r}")

    def scale(self):
        """exp(logit_scale) as a Python float (a kernel argument): read from the device once per value of the parameter."""
        key = (self.logit_scale.data_ptr(), self.logit_scale._version)
        if self._scale is None or self._scale[0] != key:
            self._scale = (key, float(torch.exp(self.logit_scale.detach().float()).item()))
        return self._scale[1]

    # ------------------------------------------------------------------------------------------------ the two tails
    def _check_pixels(self, pixel_values):
        v = self.config.vision_config
        if pixel_values is None or pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (v.num_channels, v.image_size, v.image_size):
            raise ValueError(f"HipCLIPModel: pixel_values must be [N, {v.num_channels}, {v.image_size}, {v.image_size}], got "
                             f"{None if pixel_values is None else tuple(pixel_values.shape)}")

    @torch.no_grad()
    def _embed_text(self, input_ids, seqlens, want_raw=False):
        ops._need_gpu(input_ids)
        tm = self.text_model
        hs = self._text.encode(input_ids, None if seqlens is None else seqlens.to(input_ids.device))
        return ops.clip_embed_head(hs, self._text.pooled_position(input_ids), tm.final_layer_norm.weight, tm.final_layer_norm.bias,
                                   self.config.text_config.layer_norm_eps, self.text_projection.weight, want_raw=want_raw)

    @torch.no_grad()
    def _embed_image(self, pixel_values, want_raw=False):
        ops._need_gpu(pixel_values)
        vm = self.vision_model
        hs = self._vision.encode(pixel_values, select_layer=-1)   # every layer
        return ops.clip_embed_head(hs, None, vm.post_layernorm.weight, vm.post_layernorm.bias,
                                   self.config.vision_config.layer_norm_eps, self.visual_projection.weight, want_raw=want_raw)

    # ------------------------------------------------------------------------------------------------ public
    def get_text_features(self, input_ids, attention_mask=None):
        """-> fp32 [B, P], un-normalised (`text_projection(pooled_output)`), as transformers returns it.  `attention_mask`: optional,
        right padding; under the causal mask the pad tokens behind the pooled token cannot reach it, so it only saves work."""
        seqlens = self._text.check_inputs(input_ids, attention_mask)
        return self._embed_text(input_ids, seqlens, want_raw=True).raw

    def get_image_features(self, pixel_values):
        """-> fp32 [N, P], un-normalised (`visual_projection(pooled_output)`)."""
        self._check_pixels(pixel_values)
        return self._embed_image(pixel_values, want_raw=True).raw

    def forward(self, input_ids, pixel_values, attention_mask=None):
        """-> an object with `logits_per_image` fp32 [NI, NT] = exp(logit_scale) * image_embeds @ text_embeds.T, `logits_per_text` (its
        transpose), `image_embeds` fp32 [NI, P] and `text_embeds` fp32 [NT, P] (unit L2 norm)."""
        seqlens = self._text.check_inputs(input_ids, attention_mask)
        self._check_pixels(pixel_values)
        txt = self._embed_text(input_ids, seqlens).embeds
        img = self._embed_image(pixel_values).embeds
        sel = ops.clip_select(img, txt, [img.shape[0]], [txt.shape[0]], self.scale())
        lpi = sel.logits.view(img.shape[0], txt.shape[0])
        return SimpleNamespace(logits_per_image=lpi, logits_per_text=lpi.t(), image_embeds=img, text_embeds=txt)

    def select(self, pixel_values, input_ids, images_per_group, captions_per_group, attention_mask=None):
        """The selection of `select_image` for G groups at once: group g owns the next `images_per_group[g]` rows of `pixel_values`
        and the next `captions_per_group[g]` rows of `input_ids` (Python ints, every group at least one of each).  Both towers run
        once over all rows, then one launch scores every group and picks its image.  -> `ClipSelection`."""
        si, st, _ = ops.clip_group_starts(images_per_group, captions_per_group)
        seqlens = self._text.check_inputs(input_ids, attention_mask)
        self._check_pixels(pixel_values)
        if si[-1] != pixel_values.shape[0]:
            raise ValueError(f"HipCLIPModel.select: images_per_group sums to {si[-1]} but pixel_values holds {pixel_values.shape[0]} images")
        if st[-1] != input_ids.shape[0]:
            raise ValueError(f"HipCLIPModel.select: captions_per_group sums to {st[-1]} but input_ids holds {input_ids.shape[0]} captions")
        txt = self._embed_text(input_ids, seqlens).embeds
        img = self._embed_image(pixel_values).embeds
        sel = ops.clip_select(img, txt, images_per_group, captions_per_group, self.scale())
        n, m = [int(v) for v in images_per_group], [int(v) for v in captions_per_group]
        logits = [sel.logits[sel.out_start[g]:sel.out_start[g + 1]].view(n[g], m[g]) for g in range(len(n))]
        return ClipSelection(sel.best, sel.best_logit, logits)
