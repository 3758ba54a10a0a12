"""`-m gpu`: FP8 weight-only decoding (csrc/gemv_w8.hip, ops.quantize_rows_e4m3, `GreedyDecodeSession(weights=...)`,
`model.quantize_decode_weights`).

Q1 the quantiser on the device against the rule on the CPU; K1 every e4m3fn code through the kernel; K2 the GEMV against fp64
(tests/w8_ref.py); K3 the fused forms against the unfused chain, bit for bit; K4 argument errors; S1 an FP8 session against the bf16
session on a model whose weights ARE e4m3 codes times a power of two (no quantisation error: what is left is the kernel); S2 fused /
unfused and graph / eager FP8 sessions agree bit for bit; S3 the public switch; S4 the quantisation error of ordinary random weights,
recorded."""
import pytest
import torch

from conftest import rel_l2
from w8_ref import decode_e4m3, e4m3_table, gemv_w8_ref, quantize_rows_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _codes(n, k, gen):
    """Random e4m3fn codes [n, k] (every finite code equally likely; the two NaN codes become 0)."""
    c = torch.randint(0, 256, (n, k), generator=gen, dtype=torch.uint8)
    c[(c & 0x7F) == 0x7F] = 0
    return c


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(BF)
    q = _codes(N, K, g).view(F8)
    scale = (0.5 + torch.rand(N, generator=g)) * 1e-2
    return x, q, scale, g


# ------------------------------------------------------------------------------------------------------------ Q1
@pytest.mark.parametrize("shape", [(5, 16), (37, 6160), (515, 128)])
def test_q1_quantizer_on_device_equals_the_rule_on_cpu(shape):
    from dreamllm_amd import ops
    N, K = shape
    torch.manual_seed(N)
    w = (torch.randn(N, K) * 0.02).to(BF)
    w[1] = 0                                  # an all-zero row
    w[2] = 0
    w[2, K // 3] = 1e-30                      # a row whose only entry is 1e-30
    w[3] = 0.0713                             # a row whose entries are all equal
    w[4, 0] = -3.0                            # one large entry: most of the row lands in the subnormal codes
    q_ref, s_ref = quantize_rows_ref(w)
    q, s = ops.quantize_rows_e4m3(w.to(DEV))
    assert q.dtype == F8 and s.dtype == torch.float32 and q.is_cuda
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.view(torch.uint8).cpu(), q_ref.view(torch.uint8))
    v = decode_e4m3(q_ref)
    assert not v.isnan().any() and s_ref[1] == 1 and (v[1] == 0).all() and (v[3] == 448).all() and v[2, K // 3] == 448


# ------------------------------------------------------------------------------------------------------------ K1
def test_k1_every_code_converts_exactly():
    """Row n holds code n at column 0 (the two NaN codes replaced by 0), scale 1, x = e_0, fp32 output: y[n] is the code's value,
    subnormals included; -0 gives a zero (it is added to the accumulator's +0)."""
    from dreamllm_amd import ops
    q = torch.zeros(256, 16, dtype=torch.uint8)
    q[:, 0] = torch.arange(256, dtype=torch.uint8)
    q[0x7F, 0] = 0
    q[0xFF, 0] = 0
    x = torch.zeros(1, 16, dtype=BF)
    x[0, 0] = 1
    y = ops.gemv_w8(x.to(DEV), q.view(F8).to(DEV), torch.ones(256, device=DEV), out_dtype=torch.float32)
    want = e4m3_table().clone()
    want[0x7F] = want[0xFF] = 0
    assert torch.equal(y[0].cpu().double(), want)
    # the same codes at each of a lane's 16 positions and in the second form (M > 4: x read through L1)
    for col, M in ((5, 1), (15, 1), (9, 5)):
        q2 = torch.zeros(256, 16, dtype=torch.uint8)
        q2[:, col] = q[:, 0]
        x2 = torch.zeros(M, 16, dtype=BF)
        x2[:, col] = 1
        y2 = ops.gemv_w8(x2.to(DEV), q2.view(F8).to(DEV), torch.ones(256, device=DEV), out_dtype=torch.float32)
        assert torch.equal(y2.cpu().double(), want[None].expand(M, 256)), (col, M)


# ------------------------------------------------------------------------------------------------------------ K2
K2_SHAPES = [(1, 8, 16), (2, 12, 32), (3, 37, 6160), (5, 64, 4096), (6, 33, 2064), (7, 1001, 2048), (8, 515, 128), (8, 40, 11008),
             (1, 256, 11008)]


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("M,N,K", K2_SHAPES)
def test_k2_gemv_against_fp64(M, N, K, with_residual):
    """rel_l2 < 2e-5 (fp32 output) / 4e-3 (bf16 output), the bounds of test_gemv; per element
    |y - ref| <= [2^-8 |ref| for bf16 output] + (K / 64 + 8) 2^-24 scale[n] sum_k |q h|: the bf16 rounding bound plus the worst case
    of a per-lane sequential sum followed by a six-level butterfly."""
    from dreamllm_amd import ops
    x, q, scale, g = _operands(M, N, K, 1000 * M + N)
    r = torch.randn(M, N, generator=g).to(BF) if with_residual else None
    ref, mag = gemv_w8_ref(x, q, scale, r)
    acc_tol = (K / 64 + 8) * 2.0 ** -24 * mag
    xd, qd, sd = x.to(DEV), q.to(DEV), scale.to(DEV)
    rd = r.to(DEV) if with_residual else None
    for dt, bound in ((torch.float32, 2e-5), (BF, 4e-3)):
        y = ops.gemv_w8(xd, qd, sd, residual=rd, out_dtype=dt)
        assert y.dtype == dt and y.shape == (M, N)
        yd = y.cpu().double()
        err = rel_l2(yd, ref)
        tol = acc_tol + (2.0 ** -8 * ref.abs() if dt == BF else 0)
        worst = ((yd - ref).abs() / tol.clamp_min(1e-300)).max().item()
        print(f"gemv_w8 {M}x{N}x{K} residual={with_residual} {dt}: rel_l2 {err:.3e}, worst |err| / bound {worst:.3f}")
        assert err < bound
        assert ((yd - ref).abs() <= tol).all()


# ------------------------------------------------------------------------------------------------------------ K3
def _rmsnorm_torch(x, nw, eps):
    """RMSNorm with the kernels' two roundings in torch ops (rstd summed in torch's order, not the kernels')."""
    xf = x.float()
    rstd = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return (nw.float() * (xf * rstd).to(BF).float()).to(BF)


@pytest.mark.parametrize("M,K", [(3, 4096), (8, 11008), (8, 4096)])
def test_k3_fused_forms_equal_the_unfused_chain(M, K):
    """M = 3: x staged in LDS; M = 8: the second form.  `ops.rmsnorm_fwd` covers rows of up to 8192 elements, so at K = 11008 the
    unfused chain with a norm cannot be built from it: there the folded norm is held to the bf16-output bound of K2 against
    `gemv_w8` over a torch RMSNorm (one ulp of rstd moves single bf16 roundings of h), the three forms without a norm stay
    `torch.equal`, and (8, 4096) holds the second form's folded norm to `torch.equal`."""
    from dreamllm_amd import ops
    eps = 1e-6
    g = torch.Generator().manual_seed(K + M)
    x = torch.randn(M, K, generator=g).to(BF).to(DEV)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(DEV)
    # scales that put the outputs at O(1), as the activations of a decoder are
    mk = lambda n: (_codes(n, K, g).view(F8).to(DEV), ((0.5 + torch.rand(n, generator=g)) * 1e-4).to(DEV))
    (q0, s0), (q1, s1), (q2, s2) = mk(512), mk(256), mk(256)
    (qg, sg), (qu, su) = mk(1376), mk(1376)
    exact = K <= 8192
    h = ops.rmsnorm_fwd(x, nw, eps)[0] if exact else _rmsnorm_torch(x, nw, eps)

    def same(a, b):
        if exact:
            assert torch.equal(a, b)
        else:
            assert rel_l2(a, b) < 4e-3

    # folded RMSNorm, three matrices in one launch
    fused = ops.gemv_fused_w8(x, (q0, q1, q2), (s0, s1, s2), norm_w=nw, eps=eps)
    for f, (q, s) in zip(fused, ((q0, s0), (q1, s1), (q2, s2))):
        assert f.dtype == BF
        same(f, ops.gemv_w8(h, q, s))
        assert f.float().abs().mean() > 1e-2                      # not a comparison of zeros
    # three matrices in one launch without the norm
    for f, (q, s) in zip(ops.gemv_fused_w8(x, (q0, q1, q2), (s0, s1, s2)), ((q0, s0), (q1, s1), (q2, s2))):
        assert torch.equal(f, ops.gemv_w8(x, q, s))
    # SwiGLU pair
    act = ops.gemv_fused_w8(x, (qg, qu), (sg, su), norm_w=nw, eps=eps, swiglu=True)
    same(act, ops.glu_fwd(ops.gemv_w8(h, qg, sg), ops.gemv_w8(h, qu, su), 0))
    act_plain = ops.gemv_fused_w8(x, (qg, qu), (sg, su), swiglu=True)
    assert torch.equal(act_plain, ops.glu_fwd(ops.gemv_w8(x, qg, sg), ops.gemv_w8(x, qu, su), 0))
    assert act_plain.float().abs().mean() > 1e-2
    # residual
    r = torch.randn(M, 512, generator=g).to(BF).to(DEV)
    assert torch.equal(ops.gemv_fused_w8(x, (q0,), (s0,), residual=r)[0], ops.gemv_w8(x, q0, s0, residual=r))
    # fp32 head
    head = ops.gemv_fused_w8(x, (q0,), (s0,), norm_w=nw, eps=eps, out_dtype=torch.float32)[0]
    assert head.dtype == torch.float32
    same(head, ops.gemv_w8(h, q0, s0, out_dtype=torch.float32))
    head_plain = ops.gemv_fused_w8(x, (q0,), (s0,), out_dtype=torch.float32)[0]
    assert torch.equal(head_plain, ops.gemv_w8(x, q0, s0, out_dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------ K4
def test_k4_shape_errors_launch_nothing():
    from dreamllm_amd import _lib, ops
    x, q, s, _ = _operands(1, 8, 24, 0)
    with pytest.raises(ValueError):
        ops.gemv_w8(x.to(DEV), q.to(DEV), s.to(DEV))
    with pytest.raises(ValueError):
        ops.gemv_fused_w8(x.to(DEV), (q.to(DEV),), (s.to(DEV),))
    x9, q9, s9, _ = _operands(9, 8, 32, 0)
    with pytest.raises(ValueError):
        ops.gemv_w8(x9.to(DEV), q9.to(DEV), s9.to(DEV))
    with pytest.raises(ValueError):
        ops.gemv_fused_w8(x9.to(DEV), (q9.to(DEV),), (s9.to(DEV),))
    with pytest.raises(TypeError):
        ops.gemv_w8(x9[:1].to(DEV), q9.view(torch.uint8).to(DEV), s9.to(DEV))      # codes must be float8_e4m3fn
    # the entry points themselves (no Python check in front): DLLM_ERR_SHAPE = -1, before any launch
    xd, qd, sd = x9.to(DEV), q9.to(DEV), s9.to(DEV)
    y = torch.full((9, 8), 7.0, dtype=BF, device=DEV)
    p = lambda t: None if t is None else ops._vp(t.data_ptr())
    call = lambda M, K, xx, qq, ss: _lib.call("dllm_gemv_w8", p(xx), p(qq), p(ss), p(y), None, M, 8, K, 32, 32, 8, 0, 0, ops._stream())
    assert call(9, 32, xd, qd, sd) == -1 and call(1, 24, xd, qd, sd) == -1
    assert call(1, 32, None, qd, sd) == -1 and call(1, 32, xd, None, sd) == -1 and call(1, 32, xd, qd, None) == -1
    fused = lambda M, K, ss: _lib.call("dllm_gemv_fused_w8", p(xd), None, 0.0, p(qd), None, None, p(ss), None, None, p(y), None, None,
                                       None, M, 8, 0, 0, K, 32, 32, 8, 0, 0, 0, 0, 0, ops._stream())
    assert fused(9, 32, sd) == -1 and fused(1, 24, sd) == -1 and fused(1, 32, None) == -1
    torch.cuda.synchronize()
    assert (y == 7).all()
    assert call(1, 32, xd, qd, sd) == 0                          # the same call with legal arguments runs


# ------------------------------------------------------------------------------------------------------------ sessions
def _tiny():
    from dreamllm_amd.factory import TINY, build_dreamllm
    return build_dreamllm(TINY, device=DEV, dtype=BF, with_clip=False, with_sd=False).eval()


def _decoder_linears(lm):
    for layer in lm.model.layers:
        at, mlp = layer.self_attn, layer.mlp
        yield from (at.q_proj, at.k_proj, at.v_proj, at.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj)


@pytest.fixture(scope="module")
def exact_lm():
    """TINY with every decoder Linear weight overwritten by W = q * 2^-12, q = e4m3(clamp(100 randn)), q[:, 0] = +-448: W is exact in
    bf16 (std about 0.024), the quantiser returns exactly q and 2^-12, and a power-of-two scale commutes with every rounding -- the
    bf16 and the FP8 token step compute the same function."""
    lm = _tiny()
    g = torch.Generator().manual_seed(11)
    codes = []
    with torch.no_grad():
        for lin in _decoder_linears(lm):
            q = (100 * torch.randn(lin.weight.shape, generator=g)).clamp(-448, 448).to(F8).float()
            q[:, 0] = torch.where(torch.rand(q.shape[0], generator=g) < 0.5, -448.0, 448.0)
            w = (q * 2.0 ** -12).to(BF)
            assert torch.equal(w.float(), q * 2.0 ** -12)
            lin.weight.copy_(w.to(DEV))
            codes.append(q.to(F8))
    return lm, codes


def _bf16_run(lm, ids, steps):
    """bf16 session, free running: (first token, tokens [B, steps], logits of every step)."""
    from dreamllm_amd.decode import GreedyDecodeSession
    sess = GreedyDecodeSession(lm, ids.shape[0], 64)
    first = sess.prefill(ids)
    toks, logits = [], []
    for _ in range(steps):
        toks.append(sess.generate(1)[:, 0])
        logits.append(sess.logits.clone())
    return first, torch.stack(toks, 1), logits


def _forced_fp8_logits(lm, weights, ids, first, toks, **kw):
    """FP8 session teacher-forced on the bf16 session's tokens: the logits of every step."""
    from dreamllm_amd.decode import GreedyDecodeSession
    sess = GreedyDecodeSession(lm, ids.shape[0], 64, weights=weights, **kw)
    forced = torch.cat([first[:, None], toks], 1)
    sess.prefill(ids, forced_tokens=forced, forced_mask=torch.ones_like(forced, dtype=torch.bool))
    logits = []
    for i in range(toks.shape[1]):
        assert torch.equal(sess.generate(1)[:, 0], toks[:, i])
        logits.append(sess.logits.clone())
    return logits


def test_s1_fp8_session_equals_bf16_session_on_exactly_representable_weights(exact_lm):
    """Measured on MI355X: see DESIGN.md "Decode" (FP8 weight-only decoding)."""
    from dreamllm_amd.decode import DecodeWeightsFP8
    lm, codes = exact_lm
    weights = DecodeWeightsFP8.from_model(lm)
    # the quantiser recovers the construction: exactly q and 2^-12
    got = []
    for e in weights.layers:
        got += [*zip(e["qkv_parts"], e["qkv_scale_parts"]), (e["o"], e["o_scale"]), (e["gate"], e["gate_scale"]),
                (e["up"], e["up_scale"]), (e["down"], e["down_scale"])]
    assert len(got) == len(codes)
    for (q, s), want in zip(got, codes):
        assert torch.equal(q.view(torch.uint8).cpu(), want.view(torch.uint8)) and (s == 2.0 ** -12).all()
    torch.manual_seed(3)
    ids = torch.randint(3, 30000, (3, 21), device=DEV)
    first, toks, ref_logits = _bf16_run(lm, ids, 6)
    worst = 0.0
    for lg, ref in zip(_forced_fp8_logits(lm, weights, ids, first, toks), ref_logits):
        err = rel_l2(lg, ref)
        worst = max(worst, err)
        assert err < 2e-2
        top2 = ref.float().topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 0.05
        assert torch.equal(lg.argmax(-1)[clear], ref.argmax(-1)[clear])
    print(f"S1: fp8 session against bf16 session, exactly representable weights: worst rel_l2 of the logits {worst:.3e}")


def test_s2_fp8_session_fused_unfused_graph_eager_agree(exact_lm):
    from dreamllm_amd.decode import DecodeWeightsFP8, GreedyDecodeSession
    lm, _ = exact_lm
    weights = DecodeWeightsFP8.from_model(lm)
    torch.manual_seed(4)
    ids = torch.randint(3, 30000, (3, 21), device=DEV)
    runs = {}
    for name, kw in (("graph", {}), ("unfused", dict(fused=False)), ("eager", dict(use_graph=False))):
        sess = GreedyDecodeSession(lm, 3, 64, weights=weights, **kw)
        first = sess.prefill(ids)
        rest = sess.generate(6)
        runs[name] = (first, rest, sess.out_tokens[:6].clone(), sess.logits.clone())
        if name == "graph":
            first2 = sess.prefill(ids)                       # a second prefill on the same session reproduces the run
            rest2 = sess.generate(6)
            assert torch.equal(first2, first) and torch.equal(rest2, rest) and torch.equal(sess.logits, runs[name][3])
    for name in ("unfused", "eager"):
        for a, b in zip(runs["graph"], runs[name]):
            assert torch.equal(a, b), name


def test_s3_public_switch_reaches_every_fast_path():
    from dreamllm_amd import generation, ops
    from dreamllm_amd.decode import BeamDecodeSession, DecodeWeightsFP8, GreedyDecodeSession, SampledDecodeSession
    lm = _tiny()
    torch.manual_seed(5)
    ids = torch.randint(3, 30000, (2, 9), device=DEV)
    B, S, n = 2, 9, 8
    kw = dict(max_new_tokens=n, eos_token_id=-1, pad_token_id=0)
    base = {"greedy": lm.generate(ids, **kw),
            "sample": lm.generate(ids, do_sample=True, temperature=0.9, top_k=40, generator=torch.Generator().manual_seed(7), **kw),
            "beam": lm.generate(ids, num_beams=2, **kw), "slow": lm.generate(ids, fast=False, **kw)}
    s0 = lm._decode_session[1]
    assert s0.weights is None
    holder = lm.quantize_decode_weights("fp8_e4m3")
    assert isinstance(holder, DecodeWeightsFP8) and generation.decode_weights(lm) is holder
    # greedy
    out = lm.generate(ids, **kw)
    s1 = lm._decode_session[1]
    assert s1.weights is holder
    hand = GreedyDecodeSession(lm, B, S + n + 1, vocab_limit=None, weights=holder)
    want = torch.cat([ids, hand.prefill(ids)[:, None], hand.generate(n - 1)], 1)
    assert torch.equal(out, want)
    # sampling with a seeded generator
    out = lm.generate(ids, do_sample=True, temperature=0.9, top_k=40, generator=torch.Generator().manual_seed(7), **kw)
    assert lm._decode_session[1].weights is holder
    seed = lm._draw_seed(torch.Generator().manual_seed(7))
    hand = SampledDecodeSession(lm, B, S + n + 1, 0.9, 40, 1.0, eos=-1, pad=0, vocab_limit=None, weights=holder)
    want = torch.cat([ids, hand.prefill(ids, seed=seed)[:, None], hand.generate(n - 1)], 1)
    assert torch.equal(out, want)
    # beams (do_sample left False)
    out = lm.generate(ids, num_beams=2, **kw)
    assert lm._decode_session[1].weights is holder
    hand = BeamDecodeSession(lm, B, 2, S + n + 1, eos=-1, pad=0, length_penalty=1.0, early_stopping=False, max_new=n, weights=holder)
    hand.prefill(ids)
    done = generation.run_chunked(hand, n, False, lambda k, chunk: bool(hand.beam.done.all()))
    want = ops.beam_finalize(hand.beam, done, ids, 1, S + n, -1, 0, 1.0)
    assert torch.equal(out, want)
    # the same call keeps its session; another holder replaces it
    sb = lm._decode_session[1]
    lm.generate(ids, num_beams=2, **kw)
    assert lm._decode_session[1] is sb
    # the other fast paths
    lm.greedy_generate(ids, n)
    assert lm._decode_session[1].weights is holder
    lm.sample_generate(ids, n, generator=torch.Generator().manual_seed(1))
    assert lm._decode_session[1].weights is holder
    # fast=False ignores the holder
    assert torch.equal(lm.generate(ids, fast=False, **kw), base["slow"])
    # dropped: a new session again, and the bits of a model that was never quantised
    out = lm.generate(ids, **kw)
    s2 = lm._decode_session[1]
    assert s2.weights is holder and s2 is not s0
    assert lm.quantize_decode_weights(None) is None and generation.decode_weights(lm) is None
    again = {"greedy": lm.generate(ids, **kw)}
    s3 = lm._decode_session[1]
    assert s3 is not s2 and s3.weights is None
    again["sample"] = lm.generate(ids, do_sample=True, temperature=0.9, top_k=40, generator=torch.Generator().manual_seed(7), **kw)
    again["beam"] = lm.generate(ids, num_beams=2, **kw)
    for k in again:
        assert torch.equal(again[k], base[k]), k
    with pytest.raises(ValueError):
        lm.quantize_decode_weights("int4")


def test_s4_quantisation_error_of_ordinary_weights_recorded():
    """Recorded, not bounded: this is the error of the FORMAT (about 2.6 % per Linear at N(0, 0.02) weights), not of the code.
    Measured on MI355X: see DESIGN.md "Decode" (FP8 weight-only decoding)."""
    from dreamllm_amd.decode import DecodeWeightsFP8
    lm = _tiny()
    weights = DecodeWeightsFP8.from_model(lm)
    torch.manual_seed(3)
    ids = torch.randint(3, 30000, (3, 21), device=DEV)
    first, toks, ref_logits = _bf16_run(lm, ids, 6)
    errs, agree = [], []
    for lg, ref in zip(_forced_fp8_logits(lm, weights, ids, first, toks), ref_logits):
        errs.append(rel_l2(lg, ref))
        agree.append((lg.argmax(-1) == ref.argmax(-1)).float().mean().item())
        assert torch.isfinite(lg).all()
    print(f"S4: fp8 against bf16 logits, ordinary random weights: rel_l2 mean {sum(errs) / len(errs):.3e} max {max(errs):.3e}, "
          f"top-1 agreement {sum(agree) / len(agree):.3f}")
