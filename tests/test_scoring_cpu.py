"""CPU: the host side of loglikelihood() -- the batch plan, the float64 restatement against the executed reference
(tests/golden/loglikelihood.pt, tools/make_golden_score.py) and the presence of the public entry points.  No device."""
import ctypes

import pytest
import torch

from score_ref import score_ref


# ----------------------------------------------------------------------------------------------- plan_batches
def test_plan_known_answer_three_requests():
    """Hand-checked: sorted by length (2, 5, 5 tokens; the tie keeps request order), padded to S = 5; row b * S + len(ctx) - 1 + j
    predicts continuation token j (the reference's `[-n-1:-1]` slice)."""
    from dreamllm_amd.scoring import plan_batches
    reqs = [([1, 2, 3], [4, 5]), ([1], [7]), (torch.tensor([1, 9]), torch.tensor([3, 3, 3]))]
    batches, restore = plan_batches(reqs, 100, 64)
    assert len(batches) == 1
    b = batches[0]
    assert b.input_ids.tolist() == [[1, 7, 0, 0, 0], [1, 2, 3, 4, 5], [1, 9, 3, 3, 3]]
    assert b.seqlens.tolist() == [2, 5, 5] and b.seqlens.dtype == torch.int32
    assert b.rows.tolist() == [0, 5 + 2, 5 + 3, 10 + 1, 10 + 2, 10 + 3]
    assert b.targets.tolist() == [7, 4, 5, 3, 3, 3]
    assert b.seg_start.tolist() == [0, 1, 3, 6]
    assert b.request_index.tolist() == [1, 0, 2]
    assert restore.tolist() == [1, 0, 2]
    # the row that predicts a token holds the token before it
    flat = b.input_ids.reshape(-1)
    nxt = torch.cat([flat[1:], flat[:1]])
    assert torch.equal(nxt[b.rows], b.targets)


def test_plan_budget_cuts_and_order():
    from dreamllm_amd.scoring import plan_batches
    g = torch.Generator().manual_seed(3)
    reqs = []
    for _ in range(23):
        nc, nt = int(torch.randint(1, 30, (1,), generator=g)), int(torch.randint(1, 12, (1,), generator=g))
        reqs.append((torch.randint(0, 50, (nc,), generator=g).tolist(), torch.randint(0, 50, (nt,), generator=g).tolist()))
    for tokens, rows in [(64, 64), (10 ** 6, 4), (10 ** 6, 1), (1, 64), (200, 5)]:
        batches, restore = plan_batches(reqs, tokens, rows)
        seen, planned_lens = [], []
        for b in batches:
            B, S = b.input_ids.shape
            assert B <= rows and (B * S <= tokens or B == 1)
            assert int(b.seqlens.max()) == S
            for k, i in enumerate(b.request_index.tolist()):
                ctx, cont = reqs[i]
                assert b.input_ids[k, : len(ctx) + len(cont)].tolist() == ctx + cont
                r0, r1 = b.seg_start[k], b.seg_start[k + 1]
                assert b.targets[r0:r1].tolist() == cont
                assert b.rows[r0:r1].tolist() == [k * S + len(ctx) - 1 + j for j in range(len(cont))]
            seen += b.request_index.tolist()
            planned_lens += b.seqlens.tolist()
        assert sorted(seen) == list(range(len(reqs)))
        assert planned_lens == sorted(planned_lens)                      # sorted by total length
        assert torch.tensor(seen)[restore].tolist() == list(range(len(reqs)))   # the permutation restores request order
    assert len(plan_batches(reqs, 10 ** 6, 1)[0]) == len(reqs)
    assert plan_batches([], 10, 10)[0] == []


def test_plan_rejects_bad_requests_by_name():
    from dreamllm_amd.scoring import plan_batches
    ok = ([1, 2], [3])
    for bad, what in [(([], [3]), "empty context"), (([1], []), "empty continuation"), (([1] * 6, [2] * 5), "exceed"),
                      (([1, 99], [2]), "outside"), (([1], [-1]), "outside"), ((torch.zeros(2, 2, dtype=torch.long), [1]), "1-D"), (7, "pair")]:
        with pytest.raises(ValueError, match=r"request 1\b.*" + what):
            plan_batches([ok, bad], 100, 8, max_len=10, vocab=50)
    with pytest.raises(ValueError):
        plan_batches([ok], 0, 8)


# ----------------------------------------------------------------------------------------------- restatement vs executed reference
@pytest.mark.parametrize("case", ["tiny", "big_limit", "big_full"])
def test_restatement_reproduces_the_executed_reference(golden, case):
    """score_ref (float64) on the fp32 logits rows the executed reference produced must reproduce what the reference scripts'
    arithmetic made of those rows (fp32 log_softmax + gather at [-n-1:-1], stored in the fixture) to 1e-6 absolute: fp32 against
    float64 of the same logits.  The arg-max and the greedy flag are comparisons of the same fp32 values: exact."""
    c = golden("loglikelihood.pt")[case]
    assert len(c["scored_logits"]) == (len(c["requests"]) if case == "tiny" else 1)
    checked = 0
    for i, rows in enumerate(c["scored_logits"]):
        n = rows.shape[0]
        cont = torch.tensor(c["requests"][i][1][:n])
        assert rows.dtype == torch.float32 and rows.shape[1] == c["vocab_limit"]
        r = score_ref(rows, cont)
        assert float((r["logprob"] - c["token_logprobs"][i][:n].double()).abs().max()) <= 1e-6
        assert torch.equal(r["argmax"], c["argmax"][i][:n]) and torch.equal(r["greedy"], c["greedy"][i][:n])
        top2 = rows.double().topk(2, dim=-1).values
        assert torch.equal((top2[:, 0] - top2[:, 1]).float(), c["top2_gap"][i][:n])
        assert bool(((r["rank"] == 0) == r["greedy"]).all())
        checked += n
    assert checked == (int(c["num_tokens"].sum()) if case == "tiny" else 1)
    assert float((torch.stack([t.sum() for t in c["token_logprobs"]]) - c["sum_logprob"]).abs().max()) == 0.0
    assert c["num_tokens"].tolist() == [len(k) for _, k in c["requests"]]


def test_fixture_keeps_the_bf16_reference_inside_the_caps(golden):
    """The caps the GPU test uses (10 % of the tokens, one item) are met by the reference run in bf16 itself."""
    f = golden("loglikelihood.pt")
    for case in ("tiny", "big_limit", "big_full"):
        c = f[case]
        gap, err = torch.cat(c["top2_gap"]), torch.cat(c["logit_err_bf16"])
        assert float((gap < f["gap_factor"] * err).float().mean()) <= f["max_tokens_out"]
    assert len(f["tiny"]["requests"]) == 12 and sorted(set(f["tiny"]["item_of"])) == [0, 1, 2]
    assert len({len(a) + len(b) for a, b in f["tiny"]["requests"]}) > 4      # unequal lengths


def test_restatement_ties_and_rank():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0], [0.0, -0.0, 0.0, 0.0, 0.0]])
    r = score_ref(x, torch.tensor([2, 1]))
    assert r["argmax"].tolist() == [1, 0] and r["greedy"].tolist() == [False, False] and r["rank"].tolist() == [1, 1]
    r = score_ref(x, torch.tensor([1, 7]), vocab_limit=4)
    assert r["greedy"].tolist() == [True, False] and r["rank"].tolist() == [0, -1] and r["logprob"][1] == float("-inf")


# ----------------------------------------------------------------------------------------------- public surface
def test_public_entry_points_exist():
    from dreamllm_amd import _lib, ops, scoring
    from dreamllm_amd.modeling_dreamllm import DreamLLMForCausalMLM
    from dreamllm_amd.modeling_dreamllm_sdxl import DreamLLMSDXLForCausalMLM
    for cls in (DreamLLMForCausalMLM, DreamLLMSDXLForCausalMLM):
        assert hasattr(cls, "loglikelihood") and hasattr(cls, "choice_logprobs")
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.SIGNATURES["dllm_score_rows"] == [vp, i64, i64, ci] + [vp] * 7 + [ci] + [vp] * 3
    assert _lib.SIGNATURES["dllm_score_segments"] == [vp] * 3 + [i64, i64] + [vp] * 3
    assert scoring.LoglikelihoodOutput._fields == ("sum_logprob", "num_tokens", "is_greedy", "token_logprobs")
    assert callable(ops.score_rows) and callable(ops.lm_head_score)


def test_scoring_ops_have_no_cpu_fallback():
    from dreamllm_amd import ops
    with pytest.raises(RuntimeError):
        ops.score_rows(torch.zeros(2, 8), torch.zeros(2, dtype=torch.long))
