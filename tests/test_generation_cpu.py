"""CPU: the host side of generation (`dreamllm_amd/generation.py`) -- position ids, the ragged-prompt protocol, the stopping rule,
the model-re-entry stepper against a fake model, and the one-slot session cache.  Expected values are written out by hand from the
reference loop (omni/eval/language_eval/modeling_dreamllm.py:47-109: `min_prompt_size`, `input_text_mask`) and from HF's
`prepare_inputs_for_generation`."""
from types import SimpleNamespace

import pytest
import torch

from dreamllm_amd import generation as G

PAD = 0


def test_split_ragged_prompt_unequal_right_padded():
    ids = torch.tensor([[5, 6, 7, 8, PAD],
                        [9, 10, PAD, PAD, PAD],
                        [11, 12, 13, 14, 15]])
    prompt, n_new, tokens, forced, fmask = G.split_ragged_prompt(ids, PAD, 3)
    assert torch.equal(prompt, torch.tensor([[5, 6], [9, 10], [11, 12]]))       # s0 = min_prompt_size = 2
    assert n_new == 6                                                          # total_len 5 + 3, minus s0
    assert torch.equal(tokens, torch.tensor([[5, 6, 7, 8, 0, 0, 0, 0],
                                             [9, 10, 0, 0, 0, 0, 0, 0],
                                             [11, 12, 13, 14, 15, 0, 0, 0]]))
    assert torch.equal(forced, torch.tensor([[7, 8, 0, 0, 0, 0],
                                             [0, 0, 0, 0, 0, 0],
                                             [13, 14, 15, 0, 0, 0]]))
    assert torch.equal(fmask, torch.tensor([[1, 1, 0, 0, 0, 0],                 # input_text_mask[:, 2:]
                                            [0, 0, 0, 0, 0, 0],
                                            [1, 1, 1, 0, 0, 0]], dtype=torch.bool))
    assert forced.data_ptr() == tokens[:, 2:].data_ptr()                       # a view: the result is written through `tokens`


def test_split_ragged_prompt_dense():
    ids = torch.tensor([[5, 6, 7], [8, 9, 10]])
    prompt, n_new, tokens, forced, fmask = G.split_ragged_prompt(ids, 99, 2)    # a pad id that does not occur
    assert torch.equal(prompt, ids) and n_new == 2
    assert torch.equal(tokens, torch.tensor([[5, 6, 7, 99, 99], [8, 9, 10, 99, 99]]))
    assert forced.shape == (2, 2) and not fmask.any()
    assert G.split_ragged_prompt(ids, None, 2) == (ids, 2, None, None, None)   # no protocol


@pytest.mark.parametrize("ids", [[[PAD, 5, 6], [7, 8, 9]],            # left-padded
                                 [[5, PAD, 6], [7, 8, 9]]])           # a hole
def test_split_ragged_prompt_rejects_other_layouts(ids):
    with pytest.raises(ValueError, match="right-padded"):
        G.split_ragged_prompt(torch.tensor(ids), PAD, 4)


def test_split_ragged_prompt_rejects_a_mask_as_well():
    ids = torch.tensor([[5, 6, PAD]])
    with pytest.raises(ValueError, match="not both"):
        G.split_ragged_prompt(ids, PAD, 4, attention_mask=torch.ones_like(ids))


def test_left_pad_position_ids_and_check():
    mask = torch.tensor([[0, 0, 1, 1, 1],
                         [1, 1, 1, 1, 1],
                         [0, 0, 0, 0, 1]])
    assert torch.equal(G.left_pad_position_ids(mask), torch.tensor([[1, 1, 0, 1, 2],     # pads get 1 (masked_fill)
                                                                    [0, 1, 2, 3, 4],
                                                                    [1, 1, 1, 1, 0]]))
    start, lens = G.check_left_padded(mask)
    assert start.tolist() == [2, 0, 4] and lens.tolist() == [3, 5, 1]
    ones = torch.ones(2, 4, dtype=torch.long)
    assert torch.equal(G.left_pad_position_ids(ones), torch.arange(4).expand(2, 4))
    start, lens = G.check_left_padded(ones)
    assert start.tolist() == [0, 0] and lens.tolist() == [4, 4]


@pytest.mark.parametrize("mask", [[[1, 1, 1, 0], [1, 1, 1, 1]],       # right-padded
                                  [[0, 1, 0, 1], [1, 1, 1, 1]]])      # a hole
def test_check_left_padded_rejects(mask):
    with pytest.raises(ValueError, match="SomeSession.prefill.*LEFT-padded"):
        G.check_left_padded(torch.tensor(mask), "SomeSession.prefill")


def test_stopped():
    ids = torch.zeros(2, 3, dtype=torch.long)
    seen = []

    def never(i, s):
        seen.append((i, s))
        return False

    assert G.stopped([], ids, None) is False
    assert G.stopped([never], ids, "scores") is False and seen == [(ids, "scores")]
    assert G.stopped([never, lambda i, s: True], ids, None) is True
    assert G.stopped([lambda i, s: torch.tensor([True, True])], ids, None) is True
    assert G.stopped([lambda i, s: torch.tensor([True, False])], ids, None) is False   # a tensor counts when .all()


class FakeModel:
    """Records what the stepper feeds it.  Cache entries are tagged: k[r, 0, j, 0] = 100 * (row the entry was computed in) + slot j,
    so the batch order of `past_key_values` at the next call shows any reorder."""
    V = 7

    def __init__(self):
        self.calls = []

    def __call__(self, input_ids, images=None, past_key_values=None, attention_mask=None, position_ids=None, use_cache=None,
                 return_dict=None):
        R, n = input_ids.shape
        old = 0 if past_key_values is None else past_key_values[0][0].shape[2]
        self.calls.append(SimpleNamespace(
            input_ids=input_ids.clone(), images=images, use_cache=use_cache,
            attention_mask=None if attention_mask is None else attention_mask.clone(),
            position_ids=None if position_ids is None else position_ids.clone(),
            past_rows=None if past_key_values is None else (past_key_values[0][0][:, 0, :, 0] // 100).tolist()))
        new = (100.0 * torch.arange(R)[:, None] + old + torch.arange(n)[None]).view(R, 1, n, 1)
        k = new if past_key_values is None else torch.cat([past_key_values[0][0], new], 2)
        logits = torch.arange(R * n * self.V, dtype=torch.float32).view(R, n, self.V) + len(self.calls)
        return SimpleNamespace(logits=logits, past_key_values=((k, k.clone()),))


def test_model_stepper_grows_mask_sets_positions_and_reorders_cache():
    model = FakeModel()
    prompt = torch.tensor([[0, 0, 4, 5], [0, 6, 7, 8], [9, 10, 11, 12]])
    mask = torch.tensor([[0, 0, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]])
    st = G.ModelStepper(model, prompt, "img", mask)
    c0 = model.calls[0]
    assert torch.equal(c0.input_ids, prompt) and c0.images == "img" and c0.use_cache is True and c0.past_rows is None
    assert torch.equal(c0.position_ids, torch.tensor([[1, 1, 0, 1], [1, 0, 1, 2], [0, 1, 2, 3]]))
    assert torch.equal(st.logits, (torch.arange(3 * 4 * 7, dtype=torch.float32).view(3, 4, 7) + 1)[:, -1])   # last position

    out = st.step(torch.tensor([20, 21, 22]))
    st.step(torch.tensor([30, 31, 32]), parents=torch.tensor([2, 0, 0]))
    st.step(torch.tensor([40, 41, 42]))
    assert len(model.calls) == 4 and out.shape == (3, 7)
    lens = [2, 3, 4]                                                        # valid tokens per row in the prompt
    for i, c in enumerate(model.calls[1:], start=1):
        assert c.images is None and c.use_cache is True
        assert torch.equal(c.input_ids, torch.tensor([[10 * (i + 1)], [10 * (i + 1) + 1], [10 * (i + 1) + 2]]))
        assert torch.equal(c.attention_mask, torch.cat([mask, torch.ones(3, i, dtype=mask.dtype)], 1))   # one column of ones per step
        assert c.position_ids.tolist() == [[n + i - 1] for n in lens]       # the fed token's position: valid length - 1
    # cache rows as they arrived: identity, then permuted by parents [2, 0, 0]; the permutation persists into the next step
    assert model.calls[1].past_rows == [[0] * 4, [1] * 4, [2] * 4]
    assert model.calls[2].past_rows == [[2] * 5, [0] * 5, [0] * 5]
    assert model.calls[3].past_rows == [[2] * 5 + [0], [0] * 5 + [1], [0] * 5 + [2]]
    assert torch.equal(st.logits, (torch.arange(21, dtype=torch.float32).view(3, 1, 7) + 4)[:, -1])


def test_model_stepper_without_mask_and_with_repeat():
    model = FakeModel()
    st = G.ModelStepper(model, torch.tensor([[1, 2, 3], [4, 5, 6]]), repeat=2)     # beam search: 2 rows per prompt
    assert model.calls[0].position_ids is None and model.calls[0].attention_mask is None
    assert st.logits.shape == (4, 7) and torch.equal(st.logits[0], st.logits[1]) and torch.equal(st.logits[2], st.logits[3])
    st.step(torch.tensor([7, 8, 9, 10]), parents=torch.tensor([1, 1, 2, 2]))
    c = model.calls[1]
    assert c.attention_mask is None and c.position_ids is None and c.input_ids.shape == (4, 1)
    assert c.past_rows == [[0] * 3, [0] * 3, [1] * 3, [1] * 3]                  # prompt b's cache serves rows 2b, 2b + 1


def test_cached_session():
    model = SimpleNamespace()
    built = []

    def factory(tag):
        def make():
            built.append(tag)
            return object()
        return make

    a = G.cached_session(model, ("greedy", 1, 64), factory("a"))
    assert G.cached_session(model, ("greedy", 1, 64), factory("a2")) is a and built == ["a"]   # equal key: reused, no rebuild
    assert model._decode_session == (("greedy", 1, 64), a)
    b = G.cached_session(model, ("sample", 1, 64), factory("b"))
    assert b is not a and built == ["a", "b"] and model._decode_session[1] is b                # another key replaces it
    model._decode_session = None
    c = G.cached_session(model, ("sample", 1, 64), factory("c"))
    assert c is not b and built == ["a", "b", "c"]                                             # dropped: rebuilt


def test_run_chunked_chunks_of_16_or_one_per_check():
    class Sess:
        def __init__(self):
            self.asked = []

        def generate(self, m):
            self.asked.append(m)
            return m

    s, seen = Sess(), []
    assert G.run_chunked(s, 40, False, lambda n, chunk: seen.append((n, chunk)) or False) == 40
    assert s.asked == [16, 16, 7] and seen == [(1, None), (17, 16), (33, 16), (40, 7)]
    s = Sess()
    assert G.run_chunked(s, 40, True, lambda n, chunk: n == 4) == 4 and s.asked == [1, 1, 1]
    s = Sess()
    assert G.run_chunked(s, 40, False, lambda n, chunk: True) == 1 and s.asked == []           # halted by the prefill's token
