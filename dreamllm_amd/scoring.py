"""Host side of `DreamLLMForCausalMLM.loglikelihood()`: requests -> right-padded ragged batches and the rows to score.

Pure Python over CPU tensors (no device, no kernel): tests/test_scoring_cpu.py runs it without a GPU.

The alignment is the reference scorers' own (omni/eval/language_eval/submission_scripts/submission_dev_hellaswag.py and the other
four, llama_evaluation_main/.../evaluator_utils.py:124-137): they run `model(cat(context, continuation))`, take
`log_softmax(logits)[-n-1:-1]` and gather the n continuation tokens from it -- the logits row of token s predicts token s + 1, so
continuation token j (j = 0 .. n-1) is scored by the row of position len(context) - 1 + j.
"""
from __future__ import annotations

import collections
from typing import List, Optional, Sequence, Tuple

import torch

ScoreBatch = collections.namedtuple("ScoreBatch", "input_ids seqlens rows targets seg_start request_index")
ScoreBatch.__doc__ = """One planned forward.  input_ids int64 [B, S] (right-padded with `pad_id`), seqlens int32 [B] (valid tokens per row),
rows int64 [R] (flat indices b * S + s into the [B * S] hidden states, ascending), targets int64 [R] (the token each of those rows has to
predict), seg_start int64 [B + 1] (rows [seg_start[b], seg_start[b + 1]) belong to batch row b), request_index int64 [B] (the request
each batch row came from)."""


def _as_list(x, what, i):
    if isinstance(x, torch.Tensor):
        if x.dim() != 1 or x.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"request {i}: {what} must be a 1-D integer tensor, got {tuple(x.shape)} {x.dtype}")
        return [int(v) for v in x.tolist()]
    return [int(v) for v in x]


def check_requests(requests, max_len: Optional[int] = None, vocab: Optional[int] = None) -> List[Tuple[List[int], List[int]]]:
    """(context_ids, continuation_ids) pairs (lists or 1-D LongTensors) -> lists of ints, each request checked; every failure is a
    ValueError that names the request by its index."""
    out = []
    for i, req in enumerate(requests):
        try:
            ctx, cont = req
        except (TypeError, ValueError):
            raise ValueError(f"request {i}: expected a (context_ids, continuation_ids) pair") from None
        ctx, cont = _as_list(ctx, "context", i), _as_list(cont, "continuation", i)
        if not ctx:
            raise ValueError(f"request {i}: empty context (the first continuation token is scored by the last context token: "
                             "put at least the bos token there)")
        if not cont:
            raise ValueError(f"request {i}: empty continuation (nothing to score)")
        if max_len is not None and len(ctx) + len(cont) > max_len:
            raise ValueError(f"request {i}: {len(ctx)} + {len(cont)} tokens exceed max_position_embeddings = {max_len}")
        if vocab is not None:
            bad = [t for t in ctx + cont if not 0 <= t < vocab]
            if bad:
                raise ValueError(f"request {i}: token ids {bad[:4]} outside [0, {vocab})")
        out.append((ctx, cont))
    return out


def plan_batches(requests: Sequence, max_batch_tokens: int = 8192, max_batch_rows: int = 64, *, max_len: Optional[int] = None,
                 vocab: Optional[int] = None, pad_id: int = 0):
    """Requests -> (batches, restore).

    The requests are sorted by total length (ties keep their order) and cut into right-padded batches of at most `max_batch_rows` rows
    and at most `max_batch_tokens` padded tokens (B * S; a single request longer than the budget still gets a batch of its own).
    `batches` is a list of `ScoreBatch`; results concatenated over the batches in order are in PLANNED order, and
    `concatenated[restore]` is in request order (`restore` int64 [N])."""
    if max_batch_tokens < 1 or max_batch_rows < 1:
        raise ValueError("max_batch_tokens and max_batch_rows must be positive")
    reqs = check_requests(requests, max_len, vocab)
    order = sorted(range(len(reqs)), key=lambda i: len(reqs[i][0]) + len(reqs[i][1]))
    groups, cur = [], []
    for i in order:
        n = len(reqs[i][0]) + len(reqs[i][1])   # ascending: the newcomer sets the padded length
        if cur and (len(cur) + 1 > max_batch_rows or (len(cur) + 1) * n > max_batch_tokens):
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    batches = []
    for grp in groups:
        lens = [len(reqs[i][0]) + len(reqs[i][1]) for i in grp]
        B, S = len(grp), max(lens)
        ids = torch.full((B, S), int(pad_id), dtype=torch.int64)
        rows, targets, seg = [], [], [0]
        for b, i in enumerate(grp):
            ctx, cont = reqs[i]
            ids[b, : lens[b]] = torch.tensor(ctx + cont, dtype=torch.int64)
            first = b * S + len(ctx) - 1
            rows.extend(range(first, first + len(cont)))
            targets.extend(cont)
            seg.append(len(rows))
        batches.append(ScoreBatch(ids, torch.tensor(lens, dtype=torch.int32), torch.tensor(rows, dtype=torch.int64),
                                  torch.tensor(targets, dtype=torch.int64), torch.tensor(seg, dtype=torch.int64),
                                  torch.tensor(grp, dtype=torch.int64)))
    restore = torch.empty(len(reqs), dtype=torch.int64)
    restore[torch.tensor(order, dtype=torch.int64)] = torch.arange(len(reqs), dtype=torch.int64)
    return batches, restore


LoglikelihoodOutput = collections.namedtuple("LoglikelihoodOutput", "sum_logprob num_tokens is_greedy token_logprobs")
LoglikelihoodOutput.__doc__ = """sum_logprob fp32 [N] (log p(continuation | context), natural log), num_tokens int64 [N] (continuation
lengths), is_greedy bool [N] (every continuation token is the arg-max of its row), token_logprobs (a list of N fp32 tensors, or None);
all in request order on the model's device."""
