"""CPU: the float64 restatement the CLIP scoring GPU tests rely on (tests/clip_score_ref.py) against `transformers.CLIPModel`, the
state-dict layout of `HipCLIPModel`, the selection rules on hand-made rows, and the argument checks and host wiring of
`HipCLIPModel.select` / `DreamLLMForCausalMLM.best_of_n` (which run before any device work)."""
import math
from types import SimpleNamespace

import pytest
import torch

import clip_score_ref as R


def _hip_clip(eos=2, text=None, vision=None):
    from dreamllm_amd.clip_model import HipCLIPModel
    return HipCLIPModel(dict(text_config=dict(text or R.TINY_TEXT, eos_token_id=eos), vision_config=dict(vision or R.TINY_VISION),
                             projection_dim=R.TINY_PROJ)).eval()


# ----------------------------------------------------------------------------------------------- 1. restatement vs transformers
@pytest.mark.parametrize("eos", [2, 99])
def test_restatement_matches_transformers_clip_model(eos):
    """Tiny config (hidden 128, 2 heads, 2 layers, 16 positions, projection 48), five right-padded captions of lengths 12 / 7 / 9 /
    12 / 5 and four images: the restated `logits_per_image` (causal mask only, LayerNorm on the pooled row only) within 1e-5 of the
    fp32 `CLIPModel` called WITH the padding mask, under both pooling rules."""
    hf = R.hf_clip(R.TINY_TEXT, R.TINY_VISION, R.TINY_PROJ, eos)
    ids, mask = R.captions()
    pix = torch.randn(4, 3, 56, 56, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask, pixel_values=pix)
    ref = R.clip_forward_ref(hf.state_dict(), dict(R.TINY_TEXT, eos_token_id=eos), R.TINY_VISION, ids, pix)
    assert ref["pooled_position"].tolist() == [11, 6, 8, 11, 4]
    err = float((ref["logits_per_image"] - want.logits_per_image.double()).abs().max())
    print(f"eos {eos}: max |restated - transformers| logits_per_image {err:.2e}")
    assert err <= 1e-5
    assert float((ref["text_embeds"] - want.text_embeds.double()).abs().max()) <= 1e-5
    assert float((ref["image_embeds"] - want.image_embeds.double()).abs().max()) <= 1e-5


@pytest.mark.parametrize("eos", [2, 99])
def test_pooled_position_of_the_product_matches_the_restatement(eos):
    from dreamllm_amd.clip_model import HipCLIPTextModel
    tm = HipCLIPTextModel(dict(R.TINY_TEXT, eos_token_id=eos))
    ids, _ = R.captions()
    assert tm.pooled_position(ids).tolist() == R.pooled_position_ref(ids, eos).tolist() == [11, 6, 8, 11, 4]
    ids2 = ids.clone()
    ids2[0, 3] = 99   # an earlier end-of-text id: both rules take the first
    assert tm.pooled_position(ids2).tolist()[0] == R.pooled_position_ref(ids2, eos).tolist()[0] == 3


# ----------------------------------------------------------------------------------------------- 2. state dict
def test_state_dict_is_transformers_layout():
    import dreamllm_amd
    hf = R.hf_clip(R.TINY_TEXT, R.TINY_VISION, R.TINY_PROJ, 2)
    ours = _hip_clip()
    assert isinstance(ours, dreamllm_amd.HipCLIPModel)
    assert set(ours.state_dict()) == set(hf.state_dict())
    assert {k for k, _ in ours.named_parameters()} == {k for k, _ in hf.named_parameters()}
    ours.load_state_dict(hf.state_dict(), strict=True)
    for k, v in hf.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    sd = dict(hf.state_dict())
    sd["text_model.embeddings.position_ids"] = torch.arange(16)[None]      # buffers of older checkpoints
    sd["vision_model.embeddings.position_ids"] = torch.arange(17)[None]
    ours.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError):
        ours.load_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"}, strict=True)


def test_logit_scale_stays_fp32_and_configs_are_checked():
    ours = _hip_clip().to(torch.bfloat16)
    assert ours.logit_scale.dtype == torch.float32 and ours.text_projection.weight.dtype == torch.bfloat16
    assert ours.scale() == pytest.approx(math.exp(2.6592), rel=1e-6)
    with pytest.raises(ValueError, match="head_dim"):
        _hip_clip(text=dict(R.TINY_TEXT, num_attention_heads=4))
    with pytest.raises(ValueError, match="hidden_act"):
        _hip_clip(text=dict(R.TINY_TEXT, hidden_act="relu"))
    _hip_clip(text=dict(R.TINY_TEXT, hidden_act="gelu", num_attention_heads=1))   # gelu, head_dim 128


def test_from_pretrained_reads_a_local_directory_only(tmp_path):
    import json
    from dreamllm_amd.clip_model import HipCLIPModel
    hf = R.hf_clip(R.TINY_TEXT, R.TINY_VISION, R.TINY_PROJ, 99)
    (tmp_path / "config.json").write_text(json.dumps(dict(text_config=dict(R.TINY_TEXT, eos_token_id=99), vision_config=R.TINY_VISION,
                                                           projection_dim=R.TINY_PROJ, logit_scale_init_value=2.6592)))
    torch.save(hf.state_dict(), tmp_path / "pytorch_model.bin")
    ours = HipCLIPModel.from_pretrained(str(tmp_path), dtype=torch.float32)
    assert ours.config.text_config.eos_token_id == 99
    assert torch.equal(ours.state_dict()["visual_projection.weight"], hf.state_dict()["visual_projection.weight"])
    with pytest.raises(ValueError, match="local directory"):
        HipCLIPModel.from_pretrained("openai/clip-vit-large-patch14")


# ----------------------------------------------------------------------------------------------- 3. selection rules
def _unit(rows):
    x = torch.tensor(rows, dtype=torch.float64)
    return x / x.norm(dim=-1, keepdim=True)


def test_select_restatement_rules():
    txt = _unit([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]])
    # a tie between two identical images: the lower index wins (image 1 and image 2 are the same row)
    img = _unit([[0.1, 0.2, 1.0, 0.0], [1.0, 0.5, 0.0, 0.0], [1.0, 0.5, 0.0, 0.0]])
    best, bl, logits, st = R.select_ref(img, txt, [3], [2], 100.0)
    assert best.tolist() == [1] and st.tolist() == [0]
    assert bl[0] == logits[0].max() and logits[0].shape == (3, 2)
    assert best[0] == int(torch.argmax(logits[0])) // 2
    # a NaN row is never chosen and sets status
    img2 = img.clone()
    img2[1] = math.nan
    best, bl, logits, st = R.select_ref(img2, txt, [3], [2], 100.0)
    assert best.tolist() == [2] and st.tolist() == [1] and math.isfinite(float(bl[0]))
    # +inf ranks below every finite logit too
    img3 = img.clone()
    img3[0, 0] = math.inf
    best, _, _, st = R.select_ref(img3, txt, [3], [2], 100.0)
    assert best.tolist() == [1] and st.tolist() == [1]
    # an all-NaN group returns 0; the groups next to it are not affected; n = 1, m = 1
    imgs = torch.cat([torch.full((2, 4), math.nan, dtype=torch.float64), img, _unit([[0.0, 1.0, 0.0, 0.0]])])
    txts = torch.cat([txt, txt, _unit([[0.0, 1.0, 1.0, 0.0]])])
    best, bl, logits, st = R.select_ref(imgs, txts, [2, 3, 1], [2, 2, 1], 100.0)
    assert best.tolist() == [0, 1, 0] and st.tolist() == [1, 0, 0]
    assert math.isnan(float(bl[0])) and logits[2].shape == (1, 1)
    assert float(bl[2]) == pytest.approx(100.0 / math.sqrt(2.0))


def test_embed_head_restatement_rules():
    g = torch.Generator().manual_seed(0)
    hidden = torch.randn(3, 4, 16, generator=g).bfloat16()
    hidden[2] = 0.0
    w, b = torch.ones(16).bfloat16(), torch.zeros(16).bfloat16()    # a zero row under a zero bias: LayerNorm gives zeros
    proj = torch.randn(5, 16, generator=g).bfloat16()
    emb, raw, st = R.embed_head_ref(hidden, torch.tensor([3, 99, -4]), w, b, 1e-5, proj)
    assert st.tolist() == [0, 0, 1] and bool((emb[2] == 0).all())
    assert torch.allclose(emb[:2].norm(dim=-1), torch.ones(2, dtype=torch.float64), atol=1e-12)
    want = torch.nn.functional.layer_norm(hidden[1, 3].double(), (16,), eps=1e-5) @ proj.double().t()   # 99 clamps to S - 1
    assert torch.allclose(raw[1], want, atol=1e-12)


# ----------------------------------------------------------------------------------------------- 4. argument checks
def test_select_checks_its_arguments_before_device_work():
    clip = _hip_clip()
    ids, mask = R.captions()
    pix = torch.zeros(4, 3, 56, 56)
    with pytest.raises(ValueError, match="empty"):
        clip.select(pix, ids, [4, 0], [3, 2])
    with pytest.raises(ValueError, match="empty"):
        clip.select(pix, ids, [2, 2], [5, 0])
    with pytest.raises(ValueError, match="image groups"):
        clip.select(pix, ids, [4], [3, 2])
    with pytest.raises(ValueError, match="images_per_group"):
        clip.select(pix, ids, [2, 1], [3, 2])
    with pytest.raises(ValueError, match="captions_per_group"):
        clip.select(pix, ids, [2, 2], [3, 1])
    with pytest.raises(ValueError, match="pixel_values"):
        clip.select(torch.zeros(4, 3, 32, 32), ids, [2, 2], [3, 2])
    with pytest.raises(ValueError, match="max_position_embeddings"):
        clip.select(pix, torch.ones(5, 17, dtype=torch.int64), [2, 2], [3, 2])
    holes = mask.clone()
    holes[1, 2] = 0
    with pytest.raises(ValueError, match="right-padded"):
        clip.select(pix, ids, [2, 2], [3, 2], attention_mask=holes)
    with pytest.raises(ValueError, match="right-padded"):
        clip.select(pix, ids, [2, 2], [3, 2], attention_mask=mask.flip(1))
    with pytest.raises(ValueError, match="shape of input_ids"):
        clip.forward(ids, pix, attention_mask=mask[:, :5])
    for call in (lambda: clip.select(pix, ids, [2, 2], [3, 2], attention_mask=mask), lambda: clip(ids, pix),
                 lambda: clip.get_text_features(ids, mask), lambda: clip.get_image_features(pix)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()


def test_ops_have_no_cpu_fallback():
    from dreamllm_amd import ops
    e = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="empty"):
        ops.clip_select(e, e, [4, 0], [2, 2], 1.0)
    with pytest.raises(ValueError, match="groups hold"):
        ops.clip_select(e, e, [2, 1], [2, 2], 1.0)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.clip_select(e, e, [2, 2], [3, 1], 1.0)
    h = torch.zeros(2, 3, 16).bfloat16()
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.clip_embed_head(h, None, torch.ones(16).bfloat16(), torch.zeros(16).bfloat16(), 1e-5, torch.zeros(4, 16).bfloat16())


@pytest.fixture(scope="module")
def lm():
    from dreamllm_amd.factory import TINY, TINY_DIFFUSION, build_dreamllm
    small = dict(TINY, hidden_size=128, intermediate_size=256, num_attention_heads=2)
    return build_dreamllm(small, device="cpu", dtype=torch.float32, with_clip=False, diffusion=TINY_DIFFUSION, num_dream_queries=4).eval()


def _bon_args():
    ids, mask = R.captions()
    return dict(prompt_ids=torch.randint(3, 30000, (2, 5)), negative_prompt_ids=torch.randint(3, 30000, (1, 3)), clip=_hip_clip(),
                caption_ids=ids, captions_per_prompt=[2, 3], n=3, caption_attention_mask=mask, num_inference_steps=2)


@pytest.mark.parametrize("change,name", [
    (dict(n=0), "`n` must be >= 1"), (dict(seeds=[1, 2]), "`seeds` holds 2"), (dict(captions_per_prompt=[5]), "holds 1 entries"),
    (dict(captions_per_prompt=[2, 2]), "must sum to"), (dict(captions_per_prompt=[5, 0]), "must sum to"),
    (dict(clip=SimpleNamespace()), "must be a HipCLIPModel"), (dict(negative_prompt_ids=None), "needs `negative_prompt_ids`"),
    (dict(negative_prompt_ids=torch.zeros(3, 4, dtype=torch.int64)), r"\[1, seq\] or \[batch, seq\]"),
    (dict(caption_attention_mask=R.captions()[1].flip(1)), "right-padded"),
    (dict(prompt_ids=torch.zeros(5, dtype=torch.int64)), "prompt_ids"),
])
def test_best_of_n_checks_its_arguments_before_device_work(lm, change, name):
    """CPU tensors: any device work would raise RuntimeError (no CPU fallback) -- the named ValueError must come first."""
    with pytest.raises(ValueError, match=name):
        lm.best_of_n(**dict(_bon_args(), **change))


def test_best_of_n_reaches_the_device(lm):
    with pytest.raises(RuntimeError, match="ROCm"):
        lm.best_of_n(**_bon_args())
    with pytest.raises(RuntimeError, match="ROCm"):
        lm.best_of_n(**dict(_bon_args(), negative_prompt_ids=None, guidance_scale=1.0, seeds=(7, 8, 9)))


# ----------------------------------------------------------------------------------------------- 5. host wiring of best_of_n
def test_best_of_n_host_wiring(lm, monkeypatch):
    """Stub head pipeline, stub CLIP hand-off and stub `clip.select`: the embeds are computed once per call (prompt, negative), the
    seeds arrive in order through fresh CPU generators, the images reach `select` grouped per prompt, and the gathered images are
    those at the stubbed indices."""
    from dreamllm_amd import ops
    from dreamllm_amd.generation import BestOfNOutput
    args = _bon_args()
    clip = args["clip"]
    B, n = 2, 3
    calls = dict(embeds=[], seeds=[], select=None)

    def get_prompt_embeds(ids, attention_mask=None, images=None):
        calls["embeds"].append(tuple(ids.shape))
        return torch.full((ids.shape[0], 4, 128), 1.0 if ids.shape[1] == 5 else 2.0)     # prompt / negative

    def pipeline(**kw):
        assert kw["output_type"] == "pt" and kw["num_inference_steps"] == 2 and kw["use_graph"] is True
        assert kw["prompt_embeds"].shape == (B, 4, 128) and float(kw["prompt_embeds"][0, 0, 0]) == 1.0
        assert kw["negative_prompt_embeds"].shape == (B, 4, 128) and float(kw["negative_prompt_embeds"][1, 0, 0]) == 2.0
        seed = kw["generator"].initial_seed()
        calls["seeds"].append(seed)
        return torch.stack([torch.full((3, 8, 8), seed + 0.25 * b) for b in range(B)])      # image of (seed, prompt b)

    def image_to_clip(image, size, mean, std, out_dtype=None, **kw):
        assert size == 56 and list(mean) == clip.image_mean and list(std) == clip.image_std
        return image[:, :1, :1, :1].clone()     # keeps the image's tag

    def select(pixel_values, input_ids, images_per_group, captions_per_group, attention_mask=None):
        calls["select"] = (pixel_values, input_ids, list(images_per_group), list(captions_per_group), attention_mask)
        from dreamllm_amd.clip_model import ClipSelection
        return ClipSelection(torch.tensor([2, 0]), torch.tensor([1.0, 2.0]), [torch.zeros(3, 2), torch.zeros(3, 3)])

    monkeypatch.setattr(lm, "get_prompt_embeds", get_prompt_embeds, raising=False)
    monkeypatch.setattr(lm.stable_diffusion_head, "pipeline", pipeline, raising=False)
    monkeypatch.setattr(ops, "image_to_clip", image_to_clip)
    monkeypatch.setattr(clip, "select", select, raising=False)
    out = lm.best_of_n(**dict(args, seeds=[11, 5, 8]))
    assert isinstance(out, BestOfNOutput)
    assert calls["embeds"] == [(2, 5), (1, 3)]                   # once each, not once per seed
    assert calls["seeds"] == [11, 5, 8] and out.seeds == [11, 5, 8]
    pv, ids, npg, cpg, mask = calls["select"]
    assert npg == [3, 3] and cpg == [2, 3] and torch.equal(ids, args["caption_ids"]) and torch.equal(mask, args["caption_attention_mask"])
    assert pv.flatten().tolist() == [11.0, 5.0, 8.0, 11.25, 5.25, 8.25]      # prompt-major: prompt b's n images are one group
    assert out.index.tolist() == [2, 0] and [tuple(l.shape) for l in out.logits] == [(3, 2), (3, 3)]
    assert out.images.shape == (2, 3, 8, 8)
    assert float(out.images[0, 0, 0, 0]) == 8.0 and float(out.images[1, 0, 0, 0]) == 11.25
    # default seeds: the reference's seed42 ... seed49 directories
    calls["seeds"].clear()
    monkeypatch.setattr(clip, "select", lambda *a, **k: __import__("dreamllm_amd").ClipSelection(
        torch.zeros(2, dtype=torch.int64), torch.zeros(2), [torch.zeros(8, 2), torch.zeros(8, 3)]), raising=False)
    out = lm.best_of_n(**dict(args, n=8))
    assert calls["seeds"] == list(range(42, 50)) and out.seeds == list(range(42, 50))
