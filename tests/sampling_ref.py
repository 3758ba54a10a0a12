"""fp64 restatement of the sampling rule of csrc/sample.hip (`dllm_sample_logits`) and a Python Philox4x32-10, shared by the
sampling tests.  Not collected (no `test_` prefix)."""
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123 Philox4x32 with 10 rounds: ctr (4 x uint32), key (2 x uint32) -> 4 x uint32."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_u(seed, row, step):
    """The kernel's u for (seed, row, step): key = the 64-bit seed, counter = (row, step lo, step hi, 0), u = (x0 >> 8) 2^-24."""
    seed &= (1 << 64) - 1
    step &= (1 << 64) - 1
    x0 = philox4x32_10((row, step & MASK, step >> 32, 0), (seed & MASK, seed >> 32))[0]
    return (x0 >> 8) * 2.0 ** -24


def _draw(q, keep, qz, u, tol):
    """Token of the vocabulary-order draw over the kept mass q (normalised), and why it is undecidable in fp32 ('' if it is not)."""
    q = torch.where(keep, q, torch.zeros_like(q))
    q = q / q.sum()
    cum = torch.cumsum(q, 0)
    pos = torch.nonzero(keep & (qz >= 1e-30)).flatten()   # masses fp32 can hold next to the maximum's exp(0) = 1
    cums = cum[pos]
    hit = torch.nonzero(cums > u).flatten()
    j = int(hit[0]) if hit.numel() else pos.numel() - 1
    tok = int(pos[j])
    # decided by the kept masses on either side of u: fragile only when one of them is within tol of u (u = 0 picks the first
    # positive mass whatever its size; past the last one the kernel falls back to the last positive mass, as here)
    why = ""
    tol = tol * min(u, 1.0 - u) + 1e-7   # relative to the boundary u * total (total = 1 here), at either end of [0, 1)
    if not (j == 0 or u - float(cums[j - 1]) > tol):
        why = "draw-low"
    if not (u == 0.0 or j == pos.numel() - 1 or float(cums[j]) - u > tol):
        why = "draw-high"
    if u == 0.0 and bool((keep[:tok] & (qz[:tok] > 0)).any()):
        why = "draw-underflow"
    return tok, why


def reference_sample(logits, temperature, top_k, top_p, V, u, tol=1e-5):
    """One row: logits fp32 [>= V], u float.  Returns (kept count, token, why the count is undecidable, why the token is), the
    reasons '' when decidable: a top-k boundary tie closer than 1e-6 relative, a top-p mass or a draw comparison within `tol` of
    its bound (relative to the total mass) -- what fp32 arithmetic cannot be held to.  A top-p boundary within tol makes the token
    undecidable only if the two possible kept sets draw different tokens.  Both tolerances are relative: to p, and to the distance of
    u from the nearer end of [0, 1)."""
    s = logits[:V].double() / temperature
    und_n = ""
    keep = ~torch.isnan(s)
    if 0 < top_k < V:
        srt = torch.sort(s, descending=True).values
        thr = srt[top_k - 1]
        keep = s >= thr
        below = srt[top_k:]
        below = below[below < thr]
        if below.numel() and torch.isfinite(thr) and (thr - below[0]).abs() <= 1e-6 * max(thr.abs().item(), 1e-30):
            und_n = "top-k tie"
    m = s[keep].max()
    qz = torch.where(keep, torch.exp(s - m), torch.zeros_like(s))
    q = qz / qz.sum()
    alt = None
    if top_p < 1:
        idx = torch.nonzero(keep).flatten()
        sk, qk = s[idx], q[idx]
        order = torch.argsort(sk, descending=True, stable=True)
        ss, qs = sk[order], qk[order]
        csum = torch.cumsum(qs, 0)
        # mass of strictly larger values: cumulative mass before the first element of each tie group
        first = torch.searchsorted(-ss, -ss, right=False)
        g = torch.where(first > 0, csum[(first - 1).clamp_min(0)], torch.zeros_like(csum))
        p = max(top_p, 0.0)
        kp = torch.zeros_like(keep)
        kp[idx[order]] = g <= p
        tp = tol * max(p, 1e-30)
        if ((g > 0) & ((g - p).abs() <= tp)).any():     # g == 0 (the maximum's ties) is exact in fp32 as well
            und_n = und_n or "top-p boundary"
            alt = [torch.zeros_like(keep), torch.zeros_like(keep)]
            alt[0][idx[order]] = g <= p - tp
            alt[1][idx[order]] = g <= p + tp
            alt[0] |= (s == m) & keep
        keep = kp
    tok, und_t = _draw(q, keep, qz, u, tol)
    if alt is not None and not und_t:
        toks = [_draw(q, a, qz, u, tol) for a in alt]
        if any(t != tok or w for t, w in toks):
            und_t = "top-p boundary"
    return int(keep.sum()), tok, und_n or und_t, und_t
