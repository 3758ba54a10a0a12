"""CPU: known answers of the beam-search restatement (tests/beam_ref.py) on scripted logits, and the beam arguments of
`DreamLLMForCausalMLM.generate` (checked before any device work)."""
import math

import pytest
import torch

from beam_ref import LEN_OFFSET, Hypotheses, beam_search, top_candidates


def _script(table, V):
    """logits_fn from {(step, row): probabilities}; rows not listed take (step, None), then uniform."""
    def fn(ids, t):
        rows = []
        for r in range(len(ids)):
            p = table.get((t, r), table.get((t, None), [1.0 / V] * V))
            rows.append(torch.log(torch.tensor(p, dtype=torch.float32)))
        return torch.stack(rows)
    return fn


def test_len_offset_matches_the_library():
    from dreamllm_amd import ops
    assert ops.BEAM_LEN_OFFSET == LEN_OFFSET == 1


def test_tie_rule_lower_flat_index_first():
    s = torch.tensor([[0.0, -1.0, -1.0], [-1.0, 0.0, -3.0]])
    vals, flat = top_candidates(s, 4)
    assert flat == [0, 4, 1, 2] and vals == [0.0, 0.0, -1.0, -1.0]


def test_eos_below_nb_adds_a_hypothesis():
    # step 0: eos (id 3) is the best candidate -> hypothesis "prompt only"; the next two candidates become the beams
    fn = _script({(0, None): [0.1, 0.3, 0.2, 0.4]}, 4)
    rec = beam_search(fn, [[5, 6]], 2, eos=3, max_new=1)
    assert rec["tokens"][0] == [1, 2] and rec["parents"][0] == [0, 0]
    (score, end_step, end_row, n), = [h for h in rec["hyps"][0] if h[3] == 0]
    assert (end_step, end_row, n) == (0, 0, 0)
    assert score == pytest.approx(math.log(0.4) / (0 + LEN_OFFSET), abs=1e-6)


def test_eos_at_rank_nb_or_below_is_skipped():
    table = {(0, None): [0.5, 0.3, 0.1, 0.1],
             (1, 0): [0.1, 0.05, 0.05, 0.8],    # beam 0 (score log .5): eos .4 (rank 0), id 0 .05 (rank 3)
             (1, 1): [0.6, 0.01, 0.01, 0.38]}   # beam 1 (score log .3): id 0 .18 (rank 1), eos .114 (rank 2: skipped)
    rec = beam_search(_script(table, 4), [[5, 6]], 2, eos=3, max_new=2, length_penalty=1.0)
    assert rec["cand_flat"][1][0] == [3, 4, 7, 0]
    assert rec["tokens"][1] == [0, 0] and rec["parents"][1] == [1, 0]
    hyps = rec["hyps"][0]
    eos_hyps = [h for h in hyps if h[1] == 1]
    assert len(eos_hyps) == 1
    score, end_step, end_row, n = eos_hyps[0]
    assert (end_step, end_row, n) == (1, 0, 1)
    assert score == pytest.approx(math.log(0.4) / (1 + LEN_OFFSET), abs=1e-6)


def test_hypothesis_replacement_and_worst_score():
    h = Hypotheses(2, 1.0, False, 10)
    h.add(-1.0, 0, 0, 1)
    h.add(-2.0, 1, 0, 1)
    assert h.worst == -2.0
    h.add(-1.5, 2, 0, 1)                   # replaces -2.0
    assert [b[0] for b in h.beams] == [-1.0, -1.5] and h.worst == -1.5
    h.add(-1.5, 3, 0, 1)                   # not above the worst: rejected
    assert [b[1] for b in h.beams] == [0, 2]
    h.add(-1.0, 4, 0, 1)                   # drops -1.5; two equal scores remain, in insertion order
    assert [b[1] for b in h.beams] == [0, 4] and h.worst == -1.0
    assert sorted(h.beams, key=lambda b: b[0]).pop()[1] == 4   # finalize's pop(): the later of two equal scores wins


@pytest.mark.parametrize("lp", [1.0, 0.0, -0.5])
def test_is_done_rules(lp):
    def hyps(early):
        h = Hypotheses(2, lp, early, 10)
        h.add(-4.0, 0, 0, 1)
        assert not h.is_done(-1e9, 2)      # fewer than nb hypotheses: never done
        h.add(-6.0, 0, 0, 1)
        return h
    assert hyps(True).is_done(0.0, 2)
    for early in (False, "never"):
        h = hyps(early)
        for best, gen_len in ((-5.0, 2), (-20.0, 2), (-5.0, 4), (-100.0, 3), (-7.0, 1)):
            den = 10 if (early == "never" and lp > 0) else gen_len
            assert h.is_done(best, gen_len) == (h.worst >= best / den ** lp), (early, lp, best, gen_len)
    # the three modes disagree where they should
    if lp == 1.0:
        assert hyps(False).is_done(-20.0, 2) and not hyps("never").is_done(-20.0, 2)
    if lp == 0.0:
        assert hyps(False).is_done(-7.0, 2) and not hyps(False).is_done(-5.0, 2)
    if lp == -0.5:
        assert hyps("never").is_done(-5.0, 4) == hyps(False).is_done(-5.0, 4) is True


def test_finalize_padding_order_and_a_done_batch_next_to_a_running_one():
    table = {(0, 0): [0.6, 0.3, 0.05, 0.05], (0, 1): [0.6, 0.3, 0.05, 0.05],
             (1, 0): [0.05, 0.05, 0.1, 0.8], (1, 1): [0.05, 0.05, 0.1, 0.8]}
    for t in range(3):
        for r in (2, 3):
            table[(t, r)] = [0.5, 0.29, 0.16, 0.05]
    for r in (0, 1):
        table[(2, r)] = [0.25, 0.25, 0.25, 0.25]
    rec = beam_search(_script(table, 4), [[7, 8], [9, 9]], 2, eos=3, pad=0, early_stopping=True, max_new=3,
                      num_return_sequences=2)
    assert rec["steps"] == 3 and rec["done"][-1] == [True, False]
    # batch 0 is done after step 1: its rows emit pad with parent = its beam 0
    assert rec["tokens"][2][:2] == [0, 0] and rec["parents"][2][:2] == [0, 0] and rec["beam_score"][2][:2] == [0.0, 0.0]
    # batch 1, step 1: an exact tie between flat 1 (beam 0, id 1) and flat 4 (beam 1, id 0): the lower flat index wins
    assert rec["cand_flat"][1][1][1:3] == [1, 4] and rec["cand_score"][1][1][1] == rec["cand_score"][1][1][2]
    assert rec["tokens"][1][2:] == [0, 1] and rec["parents"][1][2:] == [2, 2]
    out = rec["sequences"]
    assert out.tolist() == [[7, 8, 0, 3, 0],   # log .48 / 2: eos hypothesis, eos written after it, then pad
                            [7, 8, 1, 3, 0],   # log .24 / 2
                            [9, 9, 0, 0, 0],   # running beams added at the end (generated length 3): full width, no eos
                            [9, 9, 0, 0, 1]]


def test_output_width_is_longest_plus_one_within_max_length():
    fn = _script({(0, None): [0.1, 0.3, 0.2, 0.4], (1, None): [0.1, 0.1, 0.1, 0.7]}, 4)
    rec = beam_search(fn, [[5, 6]], 2, eos=3, pad=2, max_new=4, early_stopping=True)
    out = rec["sequences"]
    assert out.shape == (1, out.shape[1]) and out.shape[1] <= 2 + 4
    row = out[0].tolist()
    n = len(row)
    assert row[:2] == [5, 6] and (3 in row[2:] or n == 6)


@pytest.fixture(scope="module")
def lm():
    from dreamllm_amd.factory import TINY, build_dreamllm
    return build_dreamllm(TINY, device="cpu", dtype=torch.float32, with_clip=False, with_sd=False).eval()


@pytest.mark.parametrize("kw,exc,name", [
    (dict(num_beams=5, do_sample=True, temperature=0.2), NotImplementedError, "num_beams"),
    (dict(num_beams=2, num_return_sequences=3), ValueError, "num_return_sequences"),
    (dict(num_return_sequences=2), NotImplementedError, "num_return_sequences"),
    (dict(length_penalty=2.0), NotImplementedError, "length_penalty"),
    (dict(early_stopping=True), NotImplementedError, "early_stopping"),
    (dict(num_beams=3, early_stopping="sometimes"), ValueError, "early_stopping"),
    (dict(num_beams=9), NotImplementedError, "num_beams"),
    (dict(num_beams=4, num_beam_groups=2), NotImplementedError, "num_beam_groups"),
    (dict(num_beams=4, constraints=[object()]), NotImplementedError, "constraints"),
    (dict(num_beams=4, output_scores=True), NotImplementedError, "output_scores"),
    (dict(num_beams=4, return_dict_in_generate=True), NotImplementedError, "return_dict_in_generate"),
])
def test_beam_arguments_are_checked_before_device_work(lm, kw, exc, name):
    ids = torch.randint(3, 30000, (1, 5))
    with pytest.raises(exc, match=name):
        lm.generate(ids, max_new_tokens=4, **kw)


@pytest.mark.parametrize("kw", [dict(num_beams=5, do_sample=False, max_new_tokens=4),
                                dict(num_beams=5, temperature=0.2, max_new_tokens=4, length_penalty=0.5, early_stopping="never",
                                     num_return_sequences=5),
                                dict(num_beams=4, max_new_tokens=3, fast=False)])
def test_beam_generate_reaches_the_device(lm, kw):
    """Beam search is accepted (no NotImplementedError) and gets as far as the first kernel, which has no CPU fallback."""
    ids = torch.randint(3, 30000, (1, 5))
    with pytest.raises(RuntimeError, match="ROCm"):
        lm.generate(ids, **kw)
