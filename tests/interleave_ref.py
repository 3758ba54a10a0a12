"""Restatements for the interleaved-generation tests (csrc/interleave.hip, generation.interleaved_decode): the park step in plain
Python, the image hand-off as two fp64 filter matrices, the torch expression the hand-off is held to, a K/V-returning decoder
forward on the oracle's functions, and the weight edit that makes a random model emit a chosen id.  Not collected."""
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------------------------- park step
def park_ref(tok, eos, trigger, step, parked, park_step, pos, kv_len, slot, advance=True):
    """dllm_interleave_park on Python lists, in place."""
    for b in range(len(tok)):
        if parked[b] == 0:
            if eos >= 0 and tok[b] == eos:
                parked[b] = 1
            elif trigger >= 0 and tok[b] == trigger:
                parked[b] = 2
            if parked[b] != 0:
                park_step[b] = step
        if parked[b] == 0 and advance:
            pos[b] += 1
            kv_len[b] += 1
            slot[b] += 1


# ------------------------------------------------------------------------------------------------------------ image hand-off
def geometry(H, W, size):
    rh, rw = (size, size * W // H) if H <= W else (size * H // W, size)
    return rh, rw, (rh - size) // 2, (rw - size) // 2


def unit_range(x, signed_range):
    x = x.float()
    return (x / 2 + 0.5).clamp(0, 1) if signed_range else x.clamp(0, 1)


def torch_hand_off(x, size, mean, std, signed_range):
    """The definition: clamp, `interpolate(bicubic, antialias=True, align_corners=False)` of the shorter side to `size`, centre crop,
    normalise, all in fp32 on x's device."""
    H, W = x.shape[-2:]
    rh, rw, top, left = geometry(H, W, size)
    v = F.interpolate(unit_range(x, signed_range), size=(rh, rw), mode="bicubic", antialias=True, align_corners=False)
    v = v[..., top:top + size, left:left + size]
    m = torch.tensor(mean, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    return (v - m) / s


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def aa_matrix(n_in, n_out):
    """fp64 [n_out, n_in]: row i holds the antialiased bicubic taps of resized pixel i (support 2 * max(scale, 1) source pixels around
    scale * (i + 0.5), cubic convolution a = -0.5 stretched by max(scale, 1), normalised to sum 1)."""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1 else 2.0
    inv = 1.0 / scale if scale >= 1 else 1.0
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        w = [_cubic((j - c + 0.5) * inv) for j in range(lo, hi)]
        t = sum(w)
        for j, v in zip(range(lo, hi), w):
            m[i, j] = v / t
    return m


def hand_off_ref(x, size, mean, std, signed_range):
    """The hand-off restated without `interpolate`: resized = Wy @ v @ Wx^T in fp64."""
    H, W = x.shape[-2:]
    rh, rw, top, left = geometry(H, W, size)
    v = unit_range(x.cpu(), signed_range).double()
    r = aa_matrix(H, rh) @ v @ aa_matrix(W, rw).t()
    r = r[..., top:top + size, left:left + size]
    m = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return (r - m) / s


# ---------------------------------------------------------------------------------------------------- decoder forward with K/V
def oracle_cfg(model):
    cfg = model.config
    sp = cfg.special_tokens2ids_dict["additional_special_tokens"]
    return dict(num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                num_key_value_heads=cfg.num_key_value_heads, rms_norm_eps=cfg.rms_norm_eps,
                max_position_embeddings=cfg.max_position_embeddings, rope_theta=cfg.rope_theta,
                special_ids={"dream_start": sp["<dream_start>"], "im_start": sp["<im_start>"]})


def forward_kv(emb, sd, cfg):
    """oracle.llm_ref.model_forward that also returns every layer's (rotated K, V) [B, Hkv, S, D]; no padding."""
    from oracle import llm_ref as R
    B, S, H = emb.shape
    hd = H // cfg["num_attention_heads"]
    nkv = cfg["num_key_value_heads"]
    cos, sin = R.rope_tables(hd, max(cfg["max_position_embeddings"], S), cfg.get("rope_theta", 10000.0))
    pos = torch.arange(S)[None]
    mask = R.causal_mask_4d(None, B, S, emb.dtype)
    x, kvs = emb, []
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        h = R.rmsnorm(x, sd[p + "input_layernorm.weight"], cfg["rms_norm_eps"])
        k = F.linear(h, sd[p + "self_attn.k_proj.weight"]).view(B, S, nkv, hd).transpose(1, 2)
        v = F.linear(h, sd[p + "self_attn.v_proj.weight"]).view(B, S, nkv, hd).transpose(1, 2)
        k = R.apply_rope(k, k, cos.to(emb.dtype), sin.to(emb.dtype), pos)[1]
        kvs.append((k, v))
        x = R.decoder_layer(x, sd, p, cfg, cos, sin, pos, mask)
    return R.rmsnorm(x, sd["model.norm.weight"], cfg["rms_norm_eps"]), kvs


# ------------------------------------------------------------------------------------------------------------- weight edit
def fire_step(model, ids, target_id, n=6, lo=1):
    """Make greedy decoding of `ids` [1, S] emit `target_id`: run an ordinary greedy `generate`, pick a step in lo..n-1 whose top
    logit is positive, copy 1.5 x the lm_head row of the token emitted there into row `target_id`.  -> (the step at which
    `target_id` now wins: the first step whose edited logit beats the step's maximum, asserted to exist with a clear margin; the
    token whose row was copied)."""
    S = ids.shape[1]
    g = model.generate(ids, max_new_tokens=n, eos_token_id=-1)
    logits = model(input_ids=g, return_dict=True).logits[0, S - 1:S - 1 + n].float()    # step i's logits
    top = logits.max(-1).values
    cand = [i for i in range(lo, n) if float(top[i]) > 0.2]
    assert cand, top.tolist()
    c = max(cand, key=lambda i: float(top[i]))
    tok = int(g[0, S + c])
    with torch.no_grad():
        model.lm_head.weight[target_id] = (1.5 * model.lm_head.weight[tok].float()).to(model.lm_head.weight.dtype)
    fired = [i for i in range(n) if 1.5 * float(logits[i, tok]) > float(top[i])]
    assert fired and fired[0] <= c, (fired, c)
    j = fired[0]
    assert 1.5 * float(logits[j, tok]) - float(top[j]) > 0.05, "the edit must win by more than bf16 noise"
    return j, tok

