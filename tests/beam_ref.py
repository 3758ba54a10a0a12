"""Beam search restated in plain torch / Python: the rules of INTEGRATION.md "Beam search" (transformers 4.35.2 `beam_search`,
`BeamSearchScorer`, `BeamHypotheses`).  The kernel (`dllm_beam_step`, csrc/beam.hip), `decode.BeamDecodeSession` and
`DreamLLMForCausalMLM.generate(num_beams > 1)` are compared against this file."""
import torch

# tokens generated before an eos candidate (or before the step, for is_done) + LEN_OFFSET = the length the scores are divided by
LEN_OFFSET = 1


def step_scores(logits, beam_score):
    """fp32 log_softmax(logits) + beam_score, in the kernel's operation order: (x - max) - log(sum exp(x - max)) + beam_score."""
    x = logits.float()
    mx = x.max(-1, keepdim=True).values
    return ((x - mx) - torch.log(torch.exp(x - mx).sum(-1, keepdim=True))) + beam_score.float()[:, None]


def top_candidates(scores, k):
    """[nb, V] -> the top k of the flattened nb * V scores, descending; ties: the lower flat index first.  (scores, flat) lists."""
    flat = scores.reshape(-1)
    thr = torch.topk(flat, k).values[-1]
    idx = torch.nonzero(flat >= thr).view(-1).tolist()
    vals = flat[idx].tolist()
    order = sorted(range(len(idx)), key=lambda i: (-vals[i], idx[i]))[:k]
    return [vals[i] for i in order], [idx[i] for i in order]


class Hypotheses:
    """BeamHypotheses: at most nb (score, end_step, end_row, length) entries in insertion order."""

    def __init__(self, nb, length_penalty, early_stopping, max_new):
        self.nb, self.lp, self.early, self.max_new = nb, float(length_penalty), early_stopping, max_new
        self.beams = []
        self.worst = 1e9

    def add(self, score, end_step, end_row, length):
        if len(self.beams) < self.nb or score > self.worst:
            self.beams.append((score, end_step, end_row, length))
            if len(self.beams) > self.nb:
                order = sorted((s[0], i) for i, s in enumerate(self.beams))
                del self.beams[order[0][1]]
                self.worst = order[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best, gen_len):
        if len(self.beams) < self.nb:
            return False
        if self.early is True:
            return True
        den = self.max_new if (self.early == "never" and self.lp > 0.0) else gen_len
        return self.worst >= best / (den ** self.lp)


def beam_search(logits_fn, prompts, nb, eos=None, pad=0, length_penalty=1.0, early_stopping=False, max_new=8,
                num_return_sequences=1, criteria=None):
    """`logits_fn(ids, step)` -> fp32 logits [B * nb, V] for the running beams `ids` (list of B * nb token lists).  `prompts`: B
    token lists of equal length (left padding included).  `criteria(ids, None)` -> bool after each step.  Returns a dict: sequences
    (LongTensor [B * nrs, width]), steps, and per step parents / tokens (global rows), candidate scores / flat indices and beam
    scores."""
    B, S = len(prompts), len(prompts[0])
    R = B * nb
    ids = [list(prompts[r // nb]) for r in range(R)]
    bs = torch.full((R,), -1e9, dtype=torch.float32)
    bs[::nb] = 0.0
    hyps = [Hypotheses(nb, length_penalty, early_stopping, max_new) for _ in range(B)]
    done = [False] * B
    rec = dict(parents=[], tokens=[], cand_score=[], cand_flat=[], beam_score=[], done=[])
    steps = 0
    for t in range(max_new):
        logits = logits_fn(ids, t)
        V = logits.shape[1]
        sc = step_scores(logits, bs)
        par, toks, nbs, cs_all, cf_all = [0] * R, [pad] * R, [0.0] * R, [], []
        gen_len = t + LEN_OFFSET
        for b in range(B):
            cs, cf = top_candidates(sc[b * nb:(b + 1) * nb], 2 * nb)
            cs_all.append(cs)
            cf_all.append(cf)
            if done[b]:
                for j in range(nb):
                    par[b * nb + j], toks[b * nb + j], nbs[b * nb + j] = b * nb, pad, 0.0
                continue
            k = 0
            for rank, (s, f) in enumerate(zip(cs, cf)):
                beam, tok = divmod(f, V)
                if eos is not None and tok == eos:
                    if rank >= nb:
                        continue
                    hyps[b].add(float(s) / (gen_len ** float(length_penalty)), t, b * nb + beam, t)
                else:
                    par[b * nb + k], toks[b * nb + k], nbs[b * nb + k] = b * nb + beam, tok, s
                    k += 1
                if k == nb:
                    break
            done[b] = done[b] or hyps[b].is_done(float(cs[0]), gen_len)
        ids = [ids[par[r]] + [toks[r]] for r in range(R)]
        bs = torch.tensor(nbs, dtype=torch.float32)
        for key, val in (("parents", par), ("tokens", toks), ("cand_score", cs_all), ("cand_flat", cf_all),
                         ("beam_score", nbs), ("done", list(done))):
            rec[key].append(val)
        steps = t + 1
        if all(done) or (criteria is not None and criteria(torch.tensor(ids), None)):
            break
    rec.update(hyps=[list(h.beams) for h in hyps], hyp_worst=[h.worst for h in hyps])   # the store before finalize
    # finalize
    best = []
    for b in range(B):
        if not done[b]:
            for j in range(nb):
                r = b * nb + j
                hyps[b].add(float(bs[r]) / (steps ** float(length_penalty)), steps, r, steps)
        ranked = sorted(hyps[b].beams, key=lambda h: h[0])
        for _ in range(num_return_sequences):
            _, end_step, row, n = ranked.pop()
            seq = []
            for s in range(end_step - 1, end_step - 1 - n, -1):
                seq.append(rec["tokens"][s][row])
                row = rec["parents"][s][row]
            best.append(list(prompts[b]) + seq[::-1])
    width = min(max(len(x) for x in best) + 1, S + max_new)
    out = torch.full((len(best), width), pad, dtype=torch.long)
    for i, x in enumerate(best):
        out[i, :len(x)] = torch.tensor(x, dtype=torch.long)
        if len(x) < width:
            out[i, len(x)] = eos if eos is not None else pad
    rec.update(sequences=out, steps=steps)
    return rec
