"""Plain-torch float64 restatement of what the scoring kernel computes per row (csrc/score.hip): log-softmax, gather, arg-max with
lowest-index ties, rank.  Used by tests/test_scoring_cpu.py (against the executed reference) and tests/test_scoring_gpu.py (against
the kernel)."""
import torch


def score_ref(logits, targets, vocab_limit=None, cand_ids=None):
    """logits [R, C] (any float dtype, taken as given), targets int64 [R] -> dict of CPU tensors: logprob / lse / cand_logprob in
    float64, argmax int64, greedy bool, rank int64.  Only the ids below `vocab_limit` count.  A target outside [0, V) (not scored)
    gives logprob 0 (t < 0) or -inf (t >= V), greedy False, rank -1.  Ties: the lowest index is the arg-max; the rank of the target is
    the number of ids with a larger value plus the number of EARLIER ids with an equal one."""
    x = logits.detach().cpu()
    targets = targets.detach().cpu().long()
    R, C = x.shape
    V = C if vocab_limit is None else min(int(vocab_limit), C)
    x = x[:, :V].double()   # (exact: every fp32 value is a float64)
    lse = torch.logsumexp(x, dim=-1)
    mx = x.max(dim=-1).values
    col = torch.arange(V)[None, :]
    argmax = torch.where(x == mx[:, None], col, V).min(dim=-1).values
    valid = (targets >= 0) & (targets < V)
    t = torch.where(valid, targets, 0)
    xt = x.gather(1, t[:, None])
    logprob = torch.where(valid, xt[:, 0] - lse, torch.where(targets < 0, 0.0, float("-inf")).double())
    rank = (x > xt).sum(-1) + ((x == xt) & (col < t[:, None])).sum(-1)
    out = dict(logprob=logprob, lse=lse, argmax=argmax, greedy=valid & (argmax == targets), rank=torch.where(valid, rank, -1))
    if cand_ids is not None:
        out["cand_logprob"] = x[:, torch.as_tensor(cand_ids, dtype=torch.long)] - lse[:, None]
    return out
