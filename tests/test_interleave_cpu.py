"""CPU: the interface of interleaved generation, its argument errors (raised before any device work), the sequence assembly and the
restatement of the image hand-off (tests/interleave_ref.py) against the torch expression it is held to."""
import pytest
import torch

import interleave_ref as R

MEAN, STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]


def test_interface_exists():
    import dataclasses
    import inspect
    import dreamllm_amd
    from dreamllm_amd import generation
    from dreamllm_amd.modeling_dreamllm import DreamLLMForCausalMLM
    assert dreamllm_amd.InterleavedOutput is generation.InterleavedOutput
    assert [f.name for f in dataclasses.fields(dreamllm_amd.InterleavedOutput)] == ["sequences", "images", "image_positions"]
    sig = inspect.signature(DreamLLMForCausalMLM.generate_interleaved)
    names = list(sig.parameters)
    assert names[:4] == ["self", "input_ids", "images", "attention_mask"]
    for name, default in dict(max_images=4, do_sample=False, temperature=1.0, top_k=50, top_p=1.0, guidance_scale=7.5,
                              num_inference_steps=50, guidance_rescale=0.0, fast=None, use_graph=True).items():
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default, name
    assert sig.parameters["max_new_tokens"].default is inspect.Parameter.empty
    assert callable(generation.interleaved_decode)


@pytest.fixture(scope="module")
def cpu_models():
    from dreamllm_amd.factory import TINY, TINY_CLIP, TINY_DIFFUSION, build_dreamllm
    small = dict(TINY, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1)
    full = build_dreamllm(small, device="cpu", dtype=torch.float32, clip=TINY_CLIP, diffusion=TINY_DIFFUSION, num_dream_queries=4)
    text = build_dreamllm(small, device="cpu", dtype=torch.float32, clip=TINY_CLIP, with_sd=False, num_dream_queries=4)
    noclip = build_dreamllm(small, device="cpu", dtype=torch.float32, with_clip=False, diffusion=TINY_DIFFUSION, num_dream_queries=4)
    return full, text, noclip


def test_argument_errors_come_before_any_kernel_call(cpu_models, monkeypatch):
    from dreamllm_amd import _lib
    full, text, noclip = cpu_models

    def no_kernel(name, *a):
        raise AssertionError(f"kernel call {name} before the argument check")

    monkeypatch.setattr(_lib, "call", no_kernel)
    ids = torch.randint(3, 30000, (2, 6))
    neg = torch.randint(3, 30000, (1, 4))
    with pytest.raises(ValueError, match="stable_diffusion_head"):
        text.generate_interleaved(ids, max_new_tokens=8)
    with pytest.raises(ValueError, match="clip_vision_embedding"):
        noclip.generate_interleaved(ids, max_new_tokens=8, negative_prompt_ids=neg)
    del_q = full.model.dream_embedding
    try:
        del full.model.dream_embedding
        with pytest.raises(ValueError, match="dream_embedding"):
            full.generate_interleaved(ids, max_new_tokens=8, negative_prompt_ids=neg)
    finally:
        full.model.dream_embedding = del_q
    with pytest.raises(ValueError, match="negative_prompt_ids"):
        full.generate_interleaved(ids, max_new_tokens=8)                      # guidance 7.5 by default
    with pytest.raises(ValueError, match="up to 8 sequences"):
        full.generate_interleaved(torch.randint(3, 30000, (9, 6)), max_new_tokens=8, guidance_scale=1.0, fast=True)
    am = torch.ones(2, 6, dtype=torch.long)
    am[0, 4:] = 0                                                             # right-padded
    with pytest.raises(ValueError, match="LEFT-padded"):
        full.generate_interleaved(ids, attention_mask=am, max_new_tokens=8, guidance_scale=1.0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        full.generate_interleaved(ids, max_new_tokens=0, guidance_scale=1.0)
    with pytest.raises(ValueError, match="temperature"):
        full.generate_interleaved(ids, max_new_tokens=8, guidance_scale=1.0, do_sample=True, temperature=0.0)


def _layout():
    from dreamllm_amd.generation import InterleaveLayout
    return InterleaveLayout(trigger=105, placeholder=101, dream_end=106, im_start=102, im_patch=101, im_end=103, n_query=3, n_patch=2)


def test_sequence_assembly_hand_written():
    from dreamllm_amd.generation import assemble_interleaved, assemble_row, trigger_room
    lay = _layout()
    assert lay.block_len == 3 + 1 + 1 + 2 + 1
    block = [101, 101, 101, 106, 102, 101, 101, 103]
    prompts = [torch.tensor([1, 7, 8]), torch.tensor([1, 9]), torch.tensor([1])]
    # phase 0: 4 steps.  row 0 parks on the trigger at its 2nd token, row 1 runs through, row 2 parks on eos (2) at its 1st token
    p0 = torch.tensor([[11, 21, 2], [105, 22, 0], [55, 23, 0], [56, 24, 0]])
    # phase 1: only row 0 is alive; it parks on the trigger again at once (first token), then phase 2 runs to the end
    p1 = torch.tensor([[105, 0, 0], [77, 0, 0]])
    p2 = torch.tensor([[31, 0, 0], [32, 0, 0], [33, 0, 0]])
    phases = [(p0, [2, 4, 1], [True, False, False]), (p1, [1, 0, 0], [True, False, False]), (p2, [3, 0, 0], [False, False, False])]
    seqs, poss = assemble_interleaved(prompts, phases, lay)
    assert seqs[0].tolist() == [1, 7, 8, 11, 105] + block + [105] + block + [31, 32, 33]
    assert poss[0] == [4, 13] and all(int(seqs[0][p]) == 105 for p in poss[0])
    assert seqs[1].tolist() == [1, 9, 21, 22, 23, 24] and poss[1] == []
    assert seqs[2].tolist() == [1, 2] and poss[2] == []
    assert seqs[0].dtype == torch.long
    seq, pos = assemble_row(torch.tensor([5]), [([], False)], lay)
    assert seq.tolist() == [5] and pos == []
    with pytest.raises(ValueError):
        assemble_row(torch.tensor([5]), [([4, 6], True)], lay)               # an image segment ends with the trigger
    # room: trigger at index c needs c + 1 + 8 <= max_new and prompt + c + 8 <= max_positions - 1
    assert trigger_room(lay, 3, 9, 512) == 0 and trigger_room(lay, 3, 8, 512) == -1 and trigger_room(lay, 3, 100, 20) == 8


@pytest.mark.parametrize("H,W,size", [(64, 64, 14), (96, 64, 32), (67, 53, 14), (53, 67, 32), (64, 64, 224), (20, 31, 56)])
@pytest.mark.parametrize("signed", [False, True])
def test_hand_off_restatement_equals_the_torch_expression(H, W, size, signed):
    g = torch.Generator().manual_seed(H * 1000 + W + size)
    x = torch.rand(2, 3, H, W, generator=g) * 1.4 - 0.2          # some values outside [0, 1]: the clamp is exercised
    if signed:
        x = x * 2 - 1
    ref = R.torch_hand_off(x, size, MEAN, STD, signed)
    got = R.hand_off_ref(x, size, MEAN, STD, signed)
    assert ref.shape == (2, 3, size, size) and got.shape == ref.shape
    # torch computes the tap centres scale * (i + 0.5) in fp32: up to ~n_in * 2^-23 = 1e-5 source pixels off; the cubic's slope is
    # <= 1 per pixel, so a tap weight moves by <= 1e-5, the <= 2 x 5 taps that matter (the rest of a wide filter is small) move a
    # value in [0, 1] by <= 1e-4 at worst, and 1 / std ~ 3.8 scales that: 4e-4 is the worst case, errors do not all align: 1e-4
    assert float((got - ref.double()).abs().max()) < 1e-4
