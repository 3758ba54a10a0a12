"""`-m gpu`: the sampling kernel (`dllm_sample_logits`, csrc/sample.hip) against the fp64 restatement (tests/sampling_ref.py),
its Philox stream, distribution, determinism and safety; the sampled decode session and `generate` / `sample_generate`."""
import pytest
import torch

from sampling_ref import philox_u, reference_sample

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _rows(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    # logits of a trained LM's spread (a flat row over 32000 ids puts every cumulative mass within fp32 noise of its neighbours)
    x = torch.randn(B, C, generator=g) * (6.0 + 8.0 * torch.rand(B, 1, generator=g))
    x[::5, : C // 7] -= 20.0                                  # some rows with a long low tail
    x[1::7, 3] = float("-inf")                                # masked ids
    return x


@pytest.mark.parametrize("V", [65, 1000, 32000, 32008])
def test_kernel_matches_fp64_restatement(V):
    from dreamllm_amd import ops
    B, C = 64, V + 8
    undecided = total = 0
    for ci, T in enumerate([0.2, 0.8, 1.0, 1.7]):
        x = _rows(B, C, 100 * V + ci)
        xd = x.to(DEV)
        g = torch.Generator().manual_seed(ci)
        u = torch.rand(B, generator=g)
        u[0], u[1] = 0.0, 1.0 - 2.0 ** -24
        ud = u.to(DEV)
        for k in (0, 1, 50, V):
            for p in (0.0, 0.5, 0.95, 1.0):
                kept = torch.empty(B, dtype=torch.int32, device=DEV)
                status = torch.zeros(B, dtype=torch.int32, device=DEV)
                tok = ops.sample_logits(xd, T, k, p, vocab_limit=V, uniforms=ud, kept_out=kept, status=status).cpu()
                kept = kept.cpu()
                assert int(status.sum()) == 0
                assert int(tok.min()) >= 0 and int(tok.max()) < V
                for b in range(B):
                    n, t, und_n, und_t = reference_sample(x[b], T, k, p, V, float(u[b]))
                    total += 1
                    if und_n or und_t:
                        undecided += 1
                    if not und_n:
                        assert int(kept[b]) == n, (V, T, k, p, b, int(kept[b]), n)
                    if not und_t:
                        assert int(tok[b]) == t, (V, T, k, p, b, float(u[b]), int(tok[b]), t)
    print(f"V={V}: {undecided} of {total} cases undecidable in fp32")
    assert undecided < 0.01 * total


def test_philox_stream_matches_restatement():
    from dreamllm_amd import ops
    B, V = 8, 1000
    x = torch.zeros(B, V, device=DEV)
    seen = set()
    for seed in (0, 1, 12345, -7, 2 ** 62 + 3):
        for step in (0, 1, 2, 2 ** 32 + 5):
            u = torch.empty(B, device=DEV)
            ops.sample_logits(x, 1.0, seed=seed, step=step, u_out=u)
            got = u.cpu().tolist()
            want = [philox_u(seed, b, step) for b in range(B)]
            assert got == want, (seed, step)
            seen.update(got)
    assert len(seen) == 5 * 4 * B  # different across rows, steps and seeds


def test_distribution_tv_distance():
    """2^20 draws of one V = 32000 row (T 0.7, top-k 50, top-p 0.9): total-variation distance to the exact kept distribution."""
    from dreamllm_amd import ops
    V, T, k, p = 32000, 0.7, 50, 0.9
    g = torch.Generator().manual_seed(5)
    row = torch.randn(V, generator=g) * 2.0
    s = row.double() / T
    thr = torch.sort(s, descending=True).values[k - 1]
    keep = s >= thr
    q = torch.where(keep, torch.exp(s - s.max()), torch.zeros_like(s))
    q /= q.sum()
    order = torch.argsort(q, descending=True)
    csum = torch.cumsum(q[order], 0)
    before = torch.cat([torch.zeros(1, dtype=csum.dtype), csum[:-1]])
    kp = torch.zeros(V, dtype=torch.bool)
    kp[order] = (before <= p) & keep[order]
    q = torch.where(kp, q, torch.zeros_like(q))
    q /= q.sum()
    B, R = 1024, 1024
    x = row.to(DEV).expand(B, V).contiguous()
    step = torch.zeros(1, dtype=torch.long, device=DEV)
    seed = torch.tensor([99], dtype=torch.long, device=DEV)
    counts = torch.zeros(V, dtype=torch.long, device=DEV)
    tok = torch.empty(B, dtype=torch.long, device=DEV)
    for _ in range(R):
        ops.sample_logits(x, T, k, p, seed=seed, step=step, tok_out=tok, advance_step=True)
        counts += torch.bincount(tok, minlength=V)
    counts = counts.cpu().double()
    assert counts[~kp].sum() == 0
    tv = 0.5 * (counts / counts.sum() - q).abs().sum().item()
    print(f"TV distance {tv:.5f} over {int(kp.sum())} kept ids")
    assert tv <= 0.005


def test_determinism_eager_vs_graph():
    from dreamllm_amd import ops
    B, V = 8, 32000
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(1)) * 3).to(DEV)
    outs = {}
    for mode in ("eager", "graph"):
        step = torch.zeros(1, dtype=torch.long, device=DEV)
        res = torch.zeros(100, B, dtype=torch.long, device=DEV)
        u = torch.empty(B, device=DEV)
        tok = torch.empty(B, dtype=torch.long, device=DEV)
        arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
        seed = torch.tensor([3], dtype=torch.long, device=DEV)   # device tensors: nothing is copied from the host inside the capture
        run = lambda: ops.sample_logits(x, 0.8, 0, 0.95, seed=seed, step=step, out_tokens=res, tok_out=tok, u_out=u, advance_step=True,
                                        arrive=arrive)
        if mode == "graph":
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                run()
            torch.cuda.current_stream().wait_stream(s)
            step.zero_()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run()
            step.zero_()
            for _ in range(100):
                graph.replay()
        else:
            for _ in range(100):
                run()
        torch.cuda.synchronize()
        assert int(step) == 100 and int(arrive) == 0
        outs[mode] = res.cpu()
    assert torch.equal(outs["eager"], outs["graph"])
    assert len(set(outs["eager"][:, 0].tolist())) > 1  # fresh numbers on every step


def test_masked_and_nonfinite_rows():
    from dreamllm_amd import ops
    B, V = 6, 5000
    x = torch.full((B, V), float("-inf"))
    x[0, 17] = 0.0
    x[1, [5, 4000]] = 1.0
    x[2] = torch.randn(V)
    x[2, 1000] = float("nan")
    x[3] = float("-inf")
    x[4] = torch.randn(V)
    x[4, 7] = float("inf")
    x[5] = torch.randn(V)
    x[5, ::2] = float("-inf")
    xd = x.to(DEV)
    for seed in range(20):
        status = torch.zeros(B, dtype=torch.int32, device=DEV)
        tok = ops.sample_logits(xd, 1.0, seed=seed, step=seed, status=status).cpu()
        st = status.cpu().tolist()
        assert st == [0, 0, 1, 1, 1, 0]
        assert int(tok[0]) == 17 and int(tok[1]) in (5, 4000) and int(tok[5]) % 2 == 1
        assert all(0 <= int(t) < V for t in tok)


# ------------------------------------------------------------------------------------------------ session and public API
@pytest.fixture(scope="module")
def tiny():
    from dreamllm_amd.factory import TINY, build_dreamllm
    return build_dreamllm(TINY, device=DEV, dtype=BF, with_clip=False, with_sd=False).eval()


def _chain_check(sess, emitted_first, seed, nsteps, T, k, p, forced=None, fmask=None, V=None):
    """First token and every graph replay: the emitted token is the fp64 reference sample of that step's logits (u recomputed
    from seed and step), or the forced token.  Returns the number of decidable checks."""
    from collections import Counter
    V = V or sess.vocab_limit
    checked = 0
    # random-weight models give near-flat rows: many draws sit within fp32 noise of a neighbouring cumulative mass (counted, skipped)
    reasons = Counter()

    def one(logits, tok, step):
        nonlocal checked
        for b in range(sess.B):
            if fmask is not None and step < fmask.shape[1] and bool(fmask[b, step]):
                assert int(tok[b]) == int(forced[b, step])
                continue
            row = logits[b].float().cpu()
            assert bool(torch.isfinite(row[:V]).all()), (step, b)
            _, t, _, und = reference_sample(row, T, k, p, V, philox_u(seed, b, step))
            reasons[und] += 1
            if not und:
                assert int(tok[b]) == t, (step, b, int(tok[b]), t)
                checked += 1

    one(sess.first_logits, emitted_first.cpu(), 0)
    for i in range(nsteps):
        tok = sess.generate(1)[:, 0].cpu()
        one(sess.logits, tok, i + 1)
    print(f"chain T={T} k={k} p={p}: {dict(reasons)}")
    assert checked >= 0.25 * sum(reasons.values()), dict(reasons)
    return checked


@pytest.mark.parametrize("protocol", ["dense", "left", "forced"])
def test_sampled_session_chain(tiny, protocol):
    from dreamllm_amd.decode import SampledDecodeSession
    torch.manual_seed(11)
    B, S = 3, 20
    ids = torch.randint(3, 30000, (B, S), device=DEV)
    am = forced = fm = None
    if protocol == "left":
        am = torch.ones(B, S, dtype=torch.long, device=DEV)
        am[1, :4] = 0
        am[2, :9] = 0
    if protocol == "forced":
        forced = torch.randint(3, 30000, (B, 6), device=DEV)
        fm = torch.zeros(B, 6, dtype=torch.bool, device=DEV)
        fm[1, :3] = True
        fm[2, :6] = True
    for T, k, p in ((0.8, 0, 0.95), (0.2, 50, 1.0)):
        sess = SampledDecodeSession(tiny, B, S + 40, T, k, p, vocab_limit=32000)
        first = sess.prefill(ids, attention_mask=am, forced_tokens=forced, forced_mask=fm, seed=1234)
        n = _chain_check(sess, first, 1234, 16, T, k, p, forced=None if forced is None else forced.cpu(),
                         fmask=None if fm is None else fm.cpu())
        assert n >= 8


def test_greedy_settings_reproduce_greedy(tiny):
    torch.manual_seed(2)
    B, S, N = 3, 17, 12
    ids = torch.randint(3, 30000, (B, S), device=DEV)
    am = torch.ones(B, S, dtype=torch.long, device=DEV)
    am[1, :5] = 0
    for mask in (None, am):
        for fast in (True, False):
            ref = tiny.greedy_generate(ids, N, attention_mask=mask, fast=fast, vocab_limit=None)
            eos = 30001 if bool((ref[:, S:] != 30001).all()) else 30002
            a = tiny.generate(ids, attention_mask=mask, max_new_tokens=N, fast=fast, eos_token_id=eos)
            b = tiny.generate(ids, attention_mask=mask, max_new_tokens=N, fast=fast, do_sample=True, top_k=1, eos_token_id=eos)
            assert torch.equal(a, ref) and torch.equal(b, ref), (mask is None, fast)
    ref = tiny.greedy_generate(ids, N)
    assert torch.equal(tiny.sample_generate(ids, N, temperature=0), ref)


def test_reproducibility(tiny):
    torch.manual_seed(4)
    ids = torch.randint(3, 30000, (3, 15), device=DEV)
    res = {}
    for use_graph in (True, False):
        torch.manual_seed(7)
        res[use_graph] = tiny.generate(ids, do_sample=True, temperature=1.0, top_k=0, max_new_tokens=16, use_graph=use_graph,
                                       eos_token_id=-1)
    assert torch.equal(res[True], res[False])
    torch.manual_seed(8)
    other = tiny.generate(ids, do_sample=True, temperature=1.0, top_k=0, max_new_tokens=16, eos_token_id=-1)
    assert not torch.equal(other, res[True])
    ids12 = torch.randint(3, 30000, (12, 15), device=DEV)
    torch.manual_seed(9)
    a = tiny.generate(ids12, do_sample=True, temperature=1.0, max_new_tokens=8, eos_token_id=-1)
    torch.manual_seed(9)
    b = tiny.generate(ids12, do_sample=True, temperature=1.0, max_new_tokens=8, eos_token_id=-1)
    assert a.shape == (12, 23) and torch.equal(a, b)
    torch.manual_seed(5)
    c = tiny.sample_generate(ids, 10)
    torch.manual_seed(5)
    assert torch.equal(c, tiny.sample_generate(ids, 10))


def test_eos_and_stopping(tiny):
    torch.manual_seed(6)
    B, S = 3, 15
    ids = torch.randint(3, 30000, (B, S), device=DEV)
    g = tiny.greedy_generate(ids, 12, vocab_limit=None)
    eos = int(g[0, S + 3])
    first0 = int((g[0, S:] == eos).int().argmax())      # row 0 reaches eos at step <= 3
    for fast in (True, False):
        out = tiny.generate(ids, max_new_tokens=12, eos_token_id=eos, pad_token_id=0, fast=fast)
        n = out.shape[1] - S
        assert int(out[0, S + first0]) == eos and bool((out[0, S + first0 + 1:] == 0).all())
        for b in range(B):
            hit = (g[b, S:] == eos).nonzero()
            if hit.numel():
                h = int(hit[0])
                assert torch.equal(out[b, S:S + h + 1], g[b, S:S + h + 1])
        ends = [(g[b, S:] == eos).nonzero() for b in range(B)]
        if all(e.numel() for e in ends):
            assert n == max(int(e[0]) for e in ends) + 1      # trimmed where every row has finished
        else:
            assert n == 12
        calls = []

        def crit(ids_, scores):
            calls.append(scores.dtype)
            return ids_.shape[1] >= S + 5

        out = tiny.generate(ids, do_sample=True, temperature=0.7, max_new_tokens=12, stopping_criteria=[crit], fast=fast,
                            eos_token_id=-1)
        assert out.shape == (B, S + 5) and calls[-1] == torch.float32


def test_vqa_sampling_call_as_written():
    """omni/eval/vqa/vqa_inference.py:119-127 on a TINY model with the CLIP plugin: autocast, torch.compile'd model, half images."""
    from dreamllm_amd import ops
    from dreamllm_amd.factory import TINY, TINY_CLIP, build_dreamllm
    from dreamllm_amd.synthetic import make_interleaved_batch
    ops.make_dynamo_opaque()
    lm = build_dreamllm(TINY, device=DEV, dtype=BF, seed=0, clip=TINY_CLIP, with_sd=False).eval()
    batch = make_interleaved_batch(1, 160, 1, n_dream=8, n_patch=16, seed=3, device=DEV, image_size=56, dm_size=128)
    n = int(batch["attention_mask"][0].sum())
    ids = batch["input_ids"][:, :n]
    img = batch["images"]

    class Crit:
        def __init__(self):
            self.n = 0

        def __call__(self, output_ids, scores, **kw):
            self.n += 1
            return False

    crit = Crit()
    model = torch.compile(lm)
    torch.manual_seed(0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model.generate(ids, images=img.half(), do_sample=True, temperature=0.2, max_new_tokens=16, stopping_criteria=[crit])
    assert out.shape[0] == 1 and out.shape[1] <= n + 16 and torch.equal(out[:, :n], ids)
    assert crit.n == out.shape[1] - n
    assert int(out[:, n:].min()) >= 0 and int(out[:, n:].max()) < lm.config.vocab_size


def test_vicuna7b_dims_chain():
    from dreamllm_amd.decode import SampledDecodeSession
    from dreamllm_amd.factory import VICUNA_7B, build_dreamllm
    model = build_dreamllm(VICUNA_7B, device=DEV, with_clip=False, with_sd=False).eval()
    for B in (1, 8):
        ids = torch.randint(3, 32000, (B, 64), device=DEV)
        for T, k, p in ((0.2, 50, 1.0), (0.8, 0, 0.95)):
            sess = SampledDecodeSession(model, B, 64 + 40, T, k, p, vocab_limit=None)
            first = sess.prefill(ids, seed=77)
            n = _chain_check(sess, first, 77, 32, T, k, p)
            assert n >= 8 * B
            del sess
    del model
    torch.cuda.empty_cache()
