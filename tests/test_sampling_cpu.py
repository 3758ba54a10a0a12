"""CPU: the Philox4x32-10 restatement the sampling GPU tests rely on, and `DreamLLMForCausalMLM.generate`'s argument checks
(which run before any device work)."""
import pytest
import torch

from sampling_ref import philox4x32_10, philox_u, reference_sample


def test_philox_known_answers():
    """Random123's known-answer vectors for Philox4x32-10."""
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    f = 0xFFFFFFFF
    assert philox4x32_10((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    u = philox_u(12345, 3, 7)
    assert 0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24)


def test_reference_sample_rules():
    """The fp64 restatement on hand-made rows: top-k ties kept, top-p `<=` rule, vocabulary-order draw, masked ids skipped."""
    lg = torch.tensor([0.0, 2.0, 2.0, 1.0, float("-inf"), 3.0])
    assert reference_sample(lg, 1.0, 2, 1.0, 6, 0.0)[:2] == (3, 1)          # k = 2: 3.0 and both 2.0 kept, first kept id drawn
    assert reference_sample(lg, 1.0, 0, 0.0, 6, 0.999)[:2] == (1, 5)        # p = 0: the arg-max only
    assert reference_sample(lg, 1.0, 0, 1.0, 4, 0.999)[:2] == (4, 3)        # vocabulary limit 4
    n, tok, _, _ = reference_sample(lg, 1.0, 0, 1.0, 6, 0.5)
    assert n == 6 and tok != 4


@pytest.fixture(scope="module")
def lm():
    from dreamllm_amd.factory import TINY, build_dreamllm
    return build_dreamllm(TINY, device="cpu", dtype=torch.float32, with_clip=False, with_sd=False).eval()


def test_generate_exists():
    from dreamllm_amd.modeling_dreamllm import DreamLLMForCausalMLM
    assert callable(getattr(DreamLLMForCausalMLM, "generate", None))
    assert callable(getattr(DreamLLMForCausalMLM, "sample_generate", None))


@pytest.mark.parametrize("kw,name", [(dict(num_beams=5), "num_beams"), (dict(num_return_sequences=2), "num_return_sequences"),
                                     (dict(repetition_penalty=1.2), "repetition_penalty"), (dict(typical_p=0.9), "typical_p"),
                                     (dict(output_scores=True), "output_scores"),
                                     (dict(return_dict_in_generate=True), "return_dict_in_generate"),
                                     (dict(no_repeat_ngram_size=3), "no_repeat_ngram_size")])
def test_generate_rejects_unsupported_arguments_before_device_work(lm, kw, name):
    """CPU tensors: any device work would raise RuntimeError (no CPU fallback) -- the named error must come first."""
    ids = torch.randint(3, 30000, (1, 5))
    with pytest.raises(NotImplementedError, match=name):
        lm.generate(ids, do_sample=True, temperature=0.2, max_new_tokens=4, **kw)


def test_generate_rejects_unknown_keywords(lm):
    ids = torch.randint(3, 30000, (1, 5))
    with pytest.raises(TypeError, match="not_an_argument"):
        lm.generate(ids, max_new_tokens=4, not_an_argument=1)
    with pytest.raises(ValueError, match="temperature"):
        lm.generate(ids, do_sample=True, temperature=0.0, max_new_tokens=4)


def test_generate_accepts_default_valued_hf_arguments_up_to_the_device(lm):
    """HF defaults passed explicitly are not rejected: the call gets as far as the first kernel, which has no CPU fallback."""
    ids = torch.randint(3, 30000, (1, 5))
    with pytest.raises(RuntimeError, match="ROCm"):
        lm.generate(ids, max_new_tokens=4, num_beams=1, output_scores=False, use_cache=True)
