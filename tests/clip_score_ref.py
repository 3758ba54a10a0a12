"""Float64 restatement of csrc/clip_score.hip (`dllm_clip_embed_head`, `dllm_clip_select`), of the text tower's pooling rule and of
`transformers.CLIPModel.forward` over a state dict -- plain torch on the CPU, shared by tests/test_clip_score_{cpu,gpu}.py.  Every
function takes `dtype` so that the same formula can also be evaluated in fp32 (the yardstick of the kernel's fp32 arithmetic)."""
import math

import torch
import torch.nn.functional as F


def pooled_position_ref(input_ids, eos_token_id):
    """transformers 4.35 `CLIPTextTransformer`: the arg-max id when the config's eos id is the legacy 2, else the first eos."""
    out = []
    for row in input_ids.tolist():
        if eos_token_id == 2:
            out.append(row.index(max(row)))
        else:
            out.append(row.index(eos_token_id) if eos_token_id in row else 0)
    return torch.tensor(out, dtype=torch.int64)


def embed_head_ref(hidden, pos, ln_w, ln_b, eps, proj, dtype=torch.float64):
    """-> (embeds [B, P], raw [B, P], status int32 [B]) in `dtype`, from the values the tensors hold (bf16 inputs are exact in it)."""
    B, S, H = hidden.shape
    r = torch.zeros(B, dtype=torch.int64) if pos is None else pos.cpu().long().clamp(0, S - 1)
    x = hidden.cpu()[torch.arange(B), r].to(dtype)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) * torch.rsqrt(var + eps) * ln_w.cpu().to(dtype) + ln_b.cpu().to(dtype)
    raw = y @ proj.cpu().to(dtype).t()
    norm = raw.pow(2).sum(-1, keepdim=True).sqrt()
    ok = torch.isfinite(norm) & (norm > 0)
    embeds = torch.where(ok, raw / norm.where(ok, torch.ones_like(norm)), torch.zeros_like(raw))
    return embeds, raw, (~ok).flatten().to(torch.int32)


def select_ref(img, txt, images_per_group, captions_per_group, scale, dtype=torch.float64):
    """-> (best int64 [G], best_logit [G], logits: list of [n_g, m_g], status int32 [G]): non-finite logits rank below every finite
    one and set status; ties go to the lowest flat index; no finite logit: best 0, best_logit NaN."""
    img, txt = img.cpu().to(dtype), txt.cpu().to(dtype)
    best, best_logit, logits, status = [], [], [], []
    i0 = j0 = 0
    for n, m in zip(images_per_group, captions_per_group):
        lg = scale * (img[i0:i0 + n] @ txt[j0:j0 + m].t())
        i0, j0 = i0 + n, j0 + m
        flat = lg.flatten()
        fin = torch.isfinite(flat)
        if bool(fin.any()):
            q = int(torch.argmax(torch.where(fin, flat, torch.full_like(flat, -math.inf))))   # first occurrence
            best.append(q // m)
            best_logit.append(float(flat[q]))
        else:
            best.append(0)
            best_logit.append(math.nan)
        status.append(0 if bool(fin.all()) else 1)
        logits.append(lg)
    return (torch.tensor(best, dtype=torch.int64), torch.tensor(best_logit, dtype=dtype), logits, torch.tensor(status, dtype=torch.int32))


def _act(x, name):
    return x * torch.sigmoid(1.702 * x) if name == "quick_gelu" else F.gelu(x)


def _layers(x, sd, prefix, n_layers, heads, eps, act, causal):
    B, S, H = x.shape
    D = H // heads
    mask = torch.full((S, S), -math.inf, dtype=x.dtype).triu(1) if causal else None
    for i in range(n_layers):
        p = f"{prefix}.encoder.layers.{i}."
        w = lambda k: sd[p + k].to(x.dtype)
        h = F.layer_norm(x, (H,), w("layer_norm1.weight"), w("layer_norm1.bias"), eps)
        q, k, v = (F.linear(h, w(f"self_attn.{n}_proj.weight"), w(f"self_attn.{n}_proj.bias")).view(B, S, heads, D).transpose(1, 2)
                   for n in "qkv")
        s = (q @ k.transpose(-1, -2)) * D ** -0.5
        if mask is not None:
            s = s + mask
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, H)
        x = x + F.linear(o, w("self_attn.out_proj.weight"), w("self_attn.out_proj.bias"))
        h = F.layer_norm(x, (H,), w("layer_norm2.weight"), w("layer_norm2.bias"), eps)
        h = _act(F.linear(h, w("mlp.fc1.weight"), w("mlp.fc1.bias")), act)
        x = x + F.linear(h, w("mlp.fc2.weight"), w("mlp.fc2.bias"))
    return x


def clip_forward_ref(sd, text_cfg, vision_cfg, input_ids, pixel_values, dtype=torch.float64):
    """`CLIPModel.forward` restated over the state dict `sd` (transformers' key names) the way the product runs it: the text tower under
    the causal mask alone (no padding mask), `final_layer_norm` / `post_layernorm` on the pooled row only, the tail and the similarity
    through `embed_head_ref` / `select_ref`.  The configs are dicts with num_hidden_layers, num_attention_heads, layer_norm_eps,
    hidden_act (both), eos_token_id (text) and patch_size (vision).
    -> dict(logits_per_image, text_embeds, image_embeds, text_raw, image_raw, pooled_position)."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    g = lambda k: sd[k].to(dtype)
    ids = input_ids.cpu().long()
    S = ids.shape[1]
    x = g("text_model.embeddings.token_embedding.weight")[ids] + g("text_model.embeddings.position_embedding.weight")[:S]
    x = _layers(x, sd, "text_model", text_cfg["num_hidden_layers"], text_cfg["num_attention_heads"], text_cfg["layer_norm_eps"],
                text_cfg["hidden_act"], True)
    pos = pooled_position_ref(ids, text_cfg["eos_token_id"])
    te, traw, _ = embed_head_ref(x, pos, sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"],
                                 text_cfg["layer_norm_eps"], sd["text_projection.weight"], dtype)
    pv = pixel_values.cpu().to(dtype)
    N = pv.shape[0]
    pe = F.conv2d(pv, g("vision_model.embeddings.patch_embedding.weight"), stride=vision_cfg["patch_size"]).flatten(2).transpose(1, 2)
    H = pe.shape[-1]
    v = torch.cat([g("vision_model.embeddings.class_embedding").expand(N, 1, H), pe], 1) + g("vision_model.embeddings.position_embedding.weight")
    v = F.layer_norm(v, (H,), g("vision_model.pre_layrnorm.weight"), g("vision_model.pre_layrnorm.bias"), vision_cfg["layer_norm_eps"])
    v = _layers(v, sd, "vision_model", vision_cfg["num_hidden_layers"], vision_cfg["num_attention_heads"], vision_cfg["layer_norm_eps"],
                vision_cfg["hidden_act"], False)
    ie, iraw, _ = embed_head_ref(v, None, sd["vision_model.post_layernorm.weight"], sd["vision_model.post_layernorm.bias"],
                                 vision_cfg["layer_norm_eps"], sd["visual_projection.weight"], dtype)
    scale = float(torch.exp(sd["logit_scale"].double()))
    _, _, logits, _ = select_ref(ie, te, [ie.shape[0]], [te.shape[0]], scale, dtype)
    return dict(logits_per_image=logits[0], text_embeds=te, image_embeds=ie, text_raw=traw, image_raw=iraw, pooled_position=pos)


# ------------------------------------------------------------------------------------------------ shared test material
TINY_TEXT = dict(vocab_size=100, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=16, layer_norm_eps=1e-5, hidden_act="quick_gelu")
TINY_VISION = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
                   num_channels=3, layer_norm_eps=1e-5, hidden_act="quick_gelu")
TINY_PROJ = 48
CAPTION_LENGTHS = (12, 7, 9, 12, 5)


def hf_clip(text, vision, proj, eos_token_id, seed=0, round_bf16=False):
    """A `transformers.CLIPModel` built from a config made in code (nothing is read from disk), in eval mode, fp32; LayerNorm weights
    and biases are perturbed so that they matter.  `round_bf16`: every floating-point tensor but `logit_scale` is rounded to bf16 values
    (still stored in fp32), so that a bf16 copy of the model holds exactly the same weights."""
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(seed)
    cfg = CLIPConfig(text_config=dict(text, eos_token_id=eos_token_id, bos_token_id=1, pad_token_id=0, projection_dim=proj),
                     vision_config=dict(vision, projection_dim=proj), projection_dim=proj)
    model = CLIPModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            if round_bf16 and name != "logit_scale":
                p.copy_(p.bfloat16().float())
    return model


def hf_clip_from_state_dict(sd, text, vision, proj, eos_token_id):
    """A `transformers.CLIPModel` (eval, fp32, CPU) holding the values of `sd` (e.g. a bf16 `HipCLIPModel.state_dict()` from the device):
    both models then hold exactly the same weights.  transformers' own weight initialisation is skipped where the installed version
    offers the switch (it is overwritten anyway)."""
    import contextlib
    from transformers import CLIPConfig, CLIPModel
    try:
        from transformers.initialization import no_init_weights
    except ImportError:
        try:
            from transformers.modeling_utils import no_init_weights
        except ImportError:
            no_init_weights = contextlib.nullcontext
    cfg = CLIPConfig(text_config=dict(text, eos_token_id=eos_token_id, bos_token_id=1, pad_token_id=0, projection_dim=proj),
                     vision_config=dict(vision, projection_dim=proj), projection_dim=proj)
    with no_init_weights():
        model = CLIPModel(cfg).eval()
    model.load_state_dict({k: v.detach().float().cpu() for k, v in sd.items()}, strict=True)
    return model


def features(out):
    """`get_text_features` / `get_image_features` of transformers: a tensor (4.x) or an output whose `pooler_output` holds it (5.x)."""
    return out if torch.is_tensor(out) else out.pooler_output


def captions(lengths=CAPTION_LENGTHS, vocab=100, seed=3):
    """Right-padded captions: bos 1, ids in [3, vocab - 2], the end-of-text id vocab - 1 (the largest id, as in CLIP's vocabulary) at
    position length - 1, pad 0 behind it -> (input_ids int64 [B, max length], attention_mask int64)."""
    g = torch.Generator().manual_seed(seed)
    S = max(lengths)
    ids = torch.zeros(len(lengths), S, dtype=torch.int64)
    mask = torch.zeros(len(lengths), S, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, 0] = 1
        ids[b, 1:n - 1] = torch.randint(3, vocab - 1, (n - 2,), generator=g)
        ids[b, n - 1] = vocab - 1
        mask[b, :n] = 1
    return ids, mask


def distinct_captions(n=64, vocab=100, positions=16, seed=3):
    """`n` right-padded captions of lengths 3 .. positions, each ending on an id of its OWN (vocab - n + b, the largest of its row, so
    the legacy arg-max rule pools it): the pooled rows start from different token embeddings and the caption embeddings come out
    nearly orthogonal (pairwise cosine about 0.06 on the tiny text tower, against 0.5 when every caption ends on the same id)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(n, positions, dtype=torch.int64)
    mask = torch.zeros(n, positions, dtype=torch.int64)
    for b in range(n):
        L = 3 + b % (positions - 2)
        ids[b, 0] = 1
        ids[b, 1:L - 1] = torch.randint(3, vocab - n, (L - 2,), generator=g)
        ids[b, L - 1] = vocab - n + b
        mask[b, :L] = 1
    return ids, mask

