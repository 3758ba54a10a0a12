"""`-m gpu` reference tests of the HBM-bound element-wise kernels (csrc/elementwise.hip, sumpool2 of csrc/groupnorm.hip) that the
fused-equals-unfused and whole-model tests lean on: each kernel against a float64 CPU formula on the SAME inputs the kernel sees
(bf16-representable values, the very fp32 cos/sin tables), at the smallest shapes that reach each of its code paths.

Bound rules (every assertion covers ALL elements -- no sampling, no share of elements allowed to differ):

* EXACT kernels assert `torch.equal` against the torch formula: one correctly rounded fp32 add followed by one round-to-nearest
  bf16 conversion is the same on both sides.  add_bcast / add_rowgroup against `(a.float() + b.float()).to(bf16)`; gather, scatter,
  pack and unpack are copies; sumpool2 on inputs that are multiples of 2^-4 with |x| <= 8 (four of them sum exactly in fp32 in any
  order, so the result is the one bf16 rounding of the exact sum).
* SINGLE-ROUNDING bf16 outputs assert per element `|got - ref64| <= 2^-8 |ref64| + floor`: the first term is the bf16 rounding of
  the fp32 result, `floor` covers the fp32 evaluation in front of it:
    RoPE                        2^-18 (|x1| + |x2|)                   (the fused multiply-add cancels)
    activations, gradients      2^-20 max(1, |x|) max(1, |dy|)        (covers the cancellation of 1 + erf for negative gelu inputs,
                                                                       about 2^-23 |x|, with an 8x margin)
    GLU forward / backward      2^-20 max(1, |a|) max(1, |b|) max(1, |d|)   (the activation floor carried through the products
                                                                       with the other operand and the upstream gradient)
    MSE backward                2^-20 |a - b| |gs|
    softmax_rows                2^-16, and every row sums to 1 within 2^-7
  No floor had to be measured: the worst element of every check is printed (`-s`) as a fraction of its bound.
* fp32 SCALARS (MSE loss, sums of squares) assert a relative error <= 1e-5 against the float64 value: all summands are positive and
  the summation depth is about 30 fp32 additions per result at these sizes (about 2e-6).
"""
import math

import pytest
import torch

from conftest import rel_l2  # noqa: F401  -- the suite's helper module; the bounds here are per element

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
GRID_CAP = 8192 * 256   # work items of one pass of the capped grid (grid_for in csrc/elementwise.hip)


def _ops():
    from dreamllm_amd import ops
    return ops


def f64(t):
    return t.detach().cpu().double()


def bf(*shape, scale=1.0):
    return (torch.randn(*shape) * scale).to(BF)


def exact16(*shape):
    """multiples of 2^-4 in [-8, 8]: bf16-representable, and a handful of them sum exactly in fp32 in any order"""
    return (torch.randint(-128, 129, shape).float() / 16).to(BF)


def check_close(name, got, ref64, floor):
    """|got - ref64| <= 2^-8 |ref64| + floor for every element; prints the worst element as a fraction of its bound"""
    got = f64(got).reshape(ref64.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref64).abs()
    lim = 2.0 ** -8 * ref64.abs() + floor
    ratio = err / lim.clamp_min(1e-300)
    w = int(ratio.argmax())
    print(f"[elementwise] {name}: worst err/bound {ratio.flatten()[w].item():.3f} (err {err.flatten()[w].item():.3e}, "
          f"ref {ref64.flatten()[w].item():.6e})")
    bad = err > lim
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst err {err.flatten()[w].item():.3e} "
                           f"> {lim.flatten()[w].item():.3e} at flat index {w} (ref {ref64.flatten()[w].item():.6e})")


def check_scalar(name, got, ref, rtol=1e-5):
    got, ref = float(got), float(ref)
    print(f"[elementwise] {name}: got {got:.9e} ref {ref:.9e} rel {abs(got - ref) / max(abs(ref), 1e-300):.2e}")
    assert abs(got - ref) <= rtol * abs(ref), f"{name}: |{got!r} - {ref!r}| > {rtol} * |ref|"


# ================================================================================================== 1. RoPE
def rope_tables(P, D, theta=10000.0):
    inv = 1.0 / theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D)
    fr = torch.outer(torch.arange(P, dtype=torch.float32), inv)
    return fr.cos().contiguous(), fr.sin().contiguous()   # fp32 [P, D/2]: handed to the kernel as they are


def rope_ref(x, cos, sin, pos, backward=False):
    """float64 rotate-half on x [B,S,NH,D] with the kernel's own fp32 tables upcast: -> (rotated, per-element floor).
    backward: the transpose rotation, computed directly."""
    B, S, NH, D = x.shape
    h = D // 2
    if pos is None:
        pos = torch.arange(S).expand(B, S)
    pos = pos.cpu().long().expand(B, S)
    c, s = cos.double()[pos][:, :, None, :], sin.double()[pos][:, :, None, :]
    if backward:
        s = -s
    x1, x2 = f64(x[..., :h]), f64(x[..., h:])
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    fl = 2.0 ** -18 * (x1.abs() + x2.abs())
    return y, torch.cat([fl, fl], -1)


def make_pos(B, S, P):
    """non-monotonic with repeats, left-padding style zeros in front, the last table row and position 0"""
    pos = torch.randint(0, P, (B, S))
    pos[:, : min(2, S)] = 0
    pos[-1, 2:] = torch.arange(S - 2)      # a left-padded row: 0 0 0 1 2 ...
    pos[0, -1] = P - 1
    return pos


ROPE_SHAPES = [(1, 5, 1, 16),     # one vector per half
               (2, 7, 3, 32),     # NH = 3, B > 1: the tok % S index wraps when pos is None
               (3, 9, 3, 80),     # five vectors per half: a non-power-of-two i % vph
               (2, 33, 2, 128)]
ROPE_P = 48


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("posmode", ["none", "bs", "1s", "int32"])
@pytest.mark.parametrize("shape", ROPE_SHAPES)
def test_rope_matches_float64_rotate_half(shape, posmode, backward):
    ops = _ops()
    B, S, NH, D = shape
    torch.manual_seed(S * D)
    cos, sin = rope_tables(ROPE_P, D)
    x = bf(B, S, NH, D)
    pos = None if posmode == "none" else make_pos(B, S, ROPE_P)
    if posmode == "1s":
        pos = pos[:1]                       # [1, S]: expanded over the batch in rope_
    ref, fl = rope_ref(x, cos, sin, pos, backward)
    if pos is not None:
        pos = pos.to(DEV).int() if posmode == "int32" else pos.to(DEV)
    got = ops.rope_(x.to(DEV), cos.to(DEV), sin.to(DEV), pos, backward=backward)
    check_close(f"rope {shape} pos={posmode} bwd={backward}", got, ref, fl)


def test_rope_on_strided_views_of_a_packed_qkv_buffer_leaves_v_alone():
    ops = _ops()
    torch.manual_seed(1)
    B, S, Hq, Hkv, D = 2, 6, 4, 2, 32
    cos, sin = rope_tables(ROPE_P, D)
    buf = bf(B, S, Hq + 2 * Hkv, D)
    pos = make_pos(B, S, ROPE_P)
    g = buf.to(DEV)
    q, k = g[:, :, :Hq], g[:, :, Hq:Hq + Hkv]
    ops.rope_(q, cos.to(DEV), sin.to(DEV), pos.to(DEV))
    ops.rope_(k, cos.to(DEV), sin.to(DEV), pos.to(DEV))
    qr, qf = rope_ref(buf[:, :, :Hq], cos, sin, pos)
    kr, kf = rope_ref(buf[:, :, Hq:Hq + Hkv], cos, sin, pos)
    check_close("rope packed q", g[:, :, :Hq], qr, qf)
    check_close("rope packed k", g[:, :, Hq:Hq + Hkv], kr, kf)
    assert torch.equal(g[:, :, Hq + Hkv:].cpu(), buf[:, :, Hq + Hkv:]), "rope_ touched the v heads"


@pytest.mark.parametrize("strided_grad", [False, True])
def test_rope_autograd_gives_the_transpose_rotation(strided_grad):
    ops = _ops()
    torch.manual_seed(2)
    B, S, Hq, Hkv, D = 2, 7, 3, 1, 32
    cos, sin = rope_tables(ROPE_P, D)
    pos = make_pos(B, S, ROPE_P)
    q0, k0 = bf(B, S, Hq, D), bf(B, S, Hkv, D)
    if strided_grad:   # [:, :S] of a longer buffer: the batch stride is not S token strides -> RoPEFn's .contiguous() branch
        gq, gk = bf(B, S + 1, Hq, D).to(DEV)[:, :S], bf(B, S + 2, Hkv, D).to(DEV)[:, :S]
        assert not ops._uniform_tok(gq) and not ops._uniform_tok(gk)
    else:
        gq, gk = bf(B, S, Hq, D).to(DEV), bf(B, S, Hkv, D).to(DEV)
    qd, kd = q0.to(DEV).requires_grad_(True), k0.to(DEV).requires_grad_(True)
    qo, ko = ops.rope(qd.clone(), kd.clone(), cos.to(DEV), sin.to(DEV), pos.to(DEV))
    gq_keep, gk_keep = gq.clone(), gk.clone()
    torch.autograd.backward([qo, ko], [gq, gk])
    for name, out, x0, grad, up, keep in (("q", qo, q0, qd.grad, gq, gq_keep), ("k", ko, k0, kd.grad, gk, gk_keep)):
        r, fl = rope_ref(x0, cos, sin, pos)
        check_close(f"rope autograd {name} fwd", out, r, fl)
        r, fl = rope_ref(keep.cpu(), cos, sin, pos, backward=True)
        check_close(f"rope autograd d{name} strided={strided_grad}", grad, r, fl)
        assert torch.equal(up, keep), "RoPEFn.backward rotated the upstream gradient in place"


def test_rope_grid_stride():
    """T * NH * D / 16 = 2 099 200 work items > 8192 * 256: the capped grid walks a second pass"""
    ops = _ops()
    B, S, NH, D = 1, 8200, 32, 128
    assert B * S * NH * D // 16 > GRID_CAP
    torch.manual_seed(3)
    cos, sin = rope_tables(S, D)
    x = bf(B, S, NH, D)
    got = ops.rope_(x.to(DEV), cos.to(DEV), sin.to(DEV))
    ref, fl = rope_ref(x, cos, sin, None)
    check_close("rope grid-stride", got, ref, fl)


def test_rope_rejects_tables_the_kernel_would_overrun():
    """ValueError from the host-side guard only: none of these calls reaches the kernel"""
    ops = _ops()
    B, S, NH, D = 1, 5, 1, 16
    x = bf(B, S, NH, D).to(DEV)
    cos, sin = (t.to(DEV) for t in rope_tables(8, D))
    with pytest.raises(ValueError):
        ops.rope_(x, cos[:4].contiguous(), sin[:4].contiguous())            # pos=None walks S = 5 rows of a 4-row table
    with pytest.raises(ValueError):
        ops.rope_(x, *(t.to(DEV) for t in rope_tables(8, 2 * D)))          # [P, D] tables (both halves), not [P, D/2]
    with pytest.raises(ValueError):
        ops.rope_(x, cos, sin[:6].contiguous())                            # cos and sin disagree
    with pytest.raises(ValueError):
        ops.rope_(x, cos.double(), sin.double())
    with pytest.raises(ValueError):
        ops.rope_(x, cos.to(BF), sin.to(BF))
    with pytest.raises(ValueError):
        ops.rope_(x, cos, sin.t().contiguous().t())                        # right shape, wrong row pitch


def test_rope_tables_first_built_under_autocast_are_the_fp32_ones():
    """Found by the guard above: torch.einsum is on autocast's low-precision list, so a model whose first forward ran under
    torch.autocast(bf16) (generate() as the VQA evaluation calls it) cached bf16 tables, which the RoPE kernels read as fp32."""
    from dreamllm_amd.modeling_dreamllm import RotaryEmbedding
    with torch.autocast("cuda", dtype=BF):
        c, s = RotaryEmbedding(32, 64).tables(16, DEV)
    c2, s2 = RotaryEmbedding(32, 64).tables(16, DEV)
    assert c.dtype == s.dtype == torch.float32 and c.shape == s.shape == (64, 16) and c.is_contiguous() and s.is_contiguous()
    assert torch.equal(c, c2) and torch.equal(s, s2)


# ================================================================================================== 2. stand-alone activations
SQRT2 = math.sqrt(2.0)


def act_ref(mode, x):
    """float64 (value, derivative), written without the cancellations of the fp32 forms (erfc, sigmoid(-x))"""
    if mode == "gelu":
        cdf = 0.5 * torch.special.erfc(-x / SQRT2)
        return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if mode == "silu":
        s, sm = torch.sigmoid(x), torch.sigmoid(-x)
        return x * s, s * (1.0 + x * sm)
    s, sm = torch.sigmoid(1.702 * x), torch.sigmoid(-1.702 * x)
    return x * s, s + 1.702 * x * s * sm


def act_floor(x, dy=None):
    fl = 2.0 ** -20 * x.abs().clamp_min(1.0)
    return fl if dy is None else fl * dy.abs().clamp_min(1.0)


_RAMP = None


def bf16_ramp():
    """every bf16 value in [-12, 12] (both tails, +-0, the subnormals), padded with zeros to a multiple of 8"""
    global _RAMP
    if _RAMP is None:
        v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF)
        v = v[torch.isfinite(v.float()) & (v.float().abs() <= 12.0)]
        assert v.numel() == 2 * (0x4140 + 1)
        _RAMP = torch.cat([v, torch.zeros(-v.numel() % 8, dtype=BF)])
    return _RAMP


def mixed_dy(n):
    return (torch.randn(n) * 10.0 ** torch.randint(-2, 3, (n,)).float()).to(BF)


def act_inputs(kind):
    torch.manual_seed(4)
    if kind == "ramp":
        x = bf16_ramp()
    elif kind == "randn":
        x = bf(4096 + 8, scale=3.0)
    else:
        x = bf(8, scale=3.0)       # one vector
    return x, mixed_dy(x.numel())


@pytest.mark.parametrize("kind", ["ramp", "randn", "one_vector"])
@pytest.mark.parametrize("mode", ["gelu", "quick_gelu", "silu"])
def test_act_fwd_bwd_match_float64(mode, kind):
    ops = _ops()
    x, dy = act_inputs(kind)
    y, g = act_ref(mode, f64(x))
    check_close(f"act_fwd {mode} {kind}", ops.act_fwd(x.to(DEV), mode), y, act_floor(f64(x)))
    check_close(f"act_bwd {mode} {kind}", ops.act_bwd(dy.to(DEV), x.to(DEV), mode), f64(dy) * g, act_floor(f64(x), f64(dy)))


@pytest.mark.parametrize("mode", ["gelu", "quick_gelu", "silu"])
def test_act_autograd(mode):
    ops = _ops()
    torch.manual_seed(5)
    x, dy = bf(6, 40, scale=3.0), mixed_dy(240).view(6, 40)
    xd = x.to(DEV).requires_grad_(True)
    out = getattr(ops, mode)(xd)
    out.backward(dy.to(DEV))
    y, g = act_ref(mode, f64(x))
    check_close(f"ops.{mode} fwd", out, y, act_floor(f64(x)))
    check_close(f"ops.{mode} grad", xd.grad, f64(dy) * g, act_floor(f64(x), f64(dy)))


def test_act_grid_stride():
    ops = _ops()
    n = 8 * (GRID_CAP + 3)         # three vectors into the second pass of the capped grid
    torch.manual_seed(6)
    x, dy = bf(n, scale=3.0), bf(n, scale=2.0)
    y, g = act_ref("gelu", f64(x))
    xd = x.to(DEV)
    check_close("act_fwd gelu grid-stride", ops.act_fwd(xd, "gelu"), y, act_floor(f64(x)))
    check_close("act_bwd gelu grid-stride", ops.act_bwd(dy.to(DEV), xd, "gelu"), f64(dy) * g, act_floor(f64(x), f64(dy)))


def test_act_rejects_sizes_that_are_no_multiple_of_8():
    ops = _ops()
    x = bf(12).to(DEV)
    with pytest.raises(ValueError, match="bad shape"):
        ops.act_fwd(x, "silu")
    with pytest.raises(ValueError, match="bad shape"):
        ops.act_bwd(x, x, "gelu")


# ================================================================================================== 3. adds
def add_ref(a, b):
    return (a.float() + b.float()).to(BF)


@pytest.mark.parametrize("ashape,bshape", [((3, 40), (3, 40)),                 # period n: plain add
                                           ((7, 5, 24), (24,)),               # period C
                                           ((3, 257, 1024), (257, 1024)),     # period S * C: CLIP position embedding
                                           ((8, GRID_CAP // 8 + 3, 8), (GRID_CAP // 8 + 3, 8))])   # grid-stride, odd period
def test_add_bcast_is_exact(ashape, bshape):
    ops = _ops()
    torch.manual_seed(7)
    a, b = bf(*ashape), bf(*bshape)
    got = ops.add_bcast(a.to(DEV), b.to(DEV))
    assert got.shape == a.shape and torch.equal(got.cpu(), add_ref(a, b))


@pytest.mark.parametrize("C", [8, 320])
def test_add_rowgroup_is_exact(C):
    ops = _ops()
    torch.manual_seed(8)
    G, R = 3, 5
    a, b = bf(G, R, C), bf(G, C)
    got = ops.add_rowgroup(a.to(DEV), b.to(DEV))
    assert torch.equal(got.cpu(), add_ref(a, b[:, None, :]))
    assert torch.equal(got, ops.add_bcast(a.to(DEV), b.to(DEV)[:, None, :].expand(G, R, C).contiguous()))


def test_add_autograd_sums_the_broadcast_operand_in_fp32():
    ops = _ops()
    torch.manual_seed(9)
    a, b, d = bf(4, 6, 24), bf(6, 24), exact16(4, 6, 24)   # exact16: the fp32 column sum is exact in any order
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = ops.add(ad, bd)
    out.backward(d.to(DEV))
    assert torch.equal(out.cpu(), add_ref(a, b))
    assert torch.equal(ad.grad.cpu(), d)
    assert torch.equal(bd.grad.cpu(), d.double().sum(0).to(BF))
    a2 = a.to(DEV).requires_grad_(True)
    c2 = bf(4, 6, 24).to(DEV).requires_grad_(True)
    ops.add(a2, c2).backward(d.to(DEV))                      # same shape: both gradients are the upstream one
    assert torch.equal(a2.grad.cpu(), d) and torch.equal(c2.grad.cpu(), d)


def test_add_bcast_rejects_an_operand_that_does_not_tile():
    ops = _ops()
    with pytest.raises(ValueError):
        ops.add_bcast(bf(3, 8).to(DEV), bf(16).to(DEV))      # 24 % 16 != 0: used to add a wrapped operand silently


# ================================================================================================== 4. MSE
MSE_N = [1,                   # one thread
         255,                 # a partial block
         2049,                # two partials
         262145,              # 129 partials, one element per thread
         1024 * 2048 + 7]     # over the 1024-partial cap: some threads take two grid-stride passes


@pytest.mark.parametrize("n", MSE_N)
def test_mse_loss_forward_backward(n):
    ops = _ops()
    torch.manual_seed(n)
    a, b = bf(n), torch.randn(n)
    a64, b64 = f64(a), b.double()

    def run():
        ad = a.to(DEV).requires_grad_(True)
        loss = ops.mse_loss(ad, b.to(DEV))
        (loss * 3.0).backward()
        return loss.detach(), ad.grad

    loss, grad = run()
    assert loss.dtype == torch.float32 and loss.shape == ()
    check_scalar(f"mse_loss n={n}", loss, ((a64 - b64) ** 2).mean())
    gs = 2.0 * 3.0 / n
    check_close(f"mse_loss grad n={n}", grad, (a64 - b64) * gs, 2.0 ** -20 * (a64 - b64).abs() * gs)
    loss2, grad2 = run()
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2), "mse_loss is not bit-identical run to run"


def test_mse_loss_per_sample_with_a_bf16_target():
    ops = _ops()
    torch.manual_seed(10)
    B, n = 3, 4 * 650
    a, b = bf(B, 4, 650), bf(B, 4, 650)                      # bf16 target: the .float() branch of mse_loss
    w = torch.tensor([1.0, -2.0, 0.5])
    ad = a.to(DEV).requires_grad_(True)
    losses = ops.mse_loss_per_sample(ad, b.to(DEV))
    assert losses.shape == (B,) and losses.dtype == torch.float32
    (losses * w.to(DEV)).sum().backward()
    diff = f64(a) - f64(b)
    for i in range(B):
        check_scalar(f"mse_loss_per_sample[{i}]", losses[i], (diff[i] ** 2).mean())
    gs = (2.0 * w.double() / n).view(B, 1, 1)
    check_close("mse_loss_per_sample grad", ad.grad, diff * gs, 2.0 ** -20 * diff.abs() * gs.abs())


# ================================================================================================== 5. sums of squares
SUMSQ_N = [7,                                     # scalar tail only
           8 * 1024 * 3 + 5,                      # single-vector loop + tail, 4 blocks
           4 * 256 * 1024 * 8 + 8 * 1024 + 3]     # 4x-unrolled loop, single-vector remainder and tail on 256 blocks


@pytest.mark.parametrize("offset", [0, 1])        # 1: a view one element into the buffer is not 16-byte aligned -> all scalar
@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_partials_match_float64(n, dtype, offset):
    ops = _ops()
    torch.manual_seed(n + offset)
    buf = torch.randn(n + 1).to(dtype)
    x = buf.to(DEV)[offset:offset + n]
    assert (x.data_ptr() % 16 == 0) == (offset == 0)
    parts = torch.zeros(ops.SUMSQ_PARTS, dtype=torch.float32, device=DEV)
    ops.sumsq_partials_(x, parts)
    ref = (f64(buf[offset:offset + n]) ** 2).sum()
    check_scalar(f"sumsq n={n} {dtype} off={offset}", ops.reduce_sum_f32(parts), ref)
    blocks = min(256, -(-n // (8 * 1024)))
    p = parts.cpu()
    assert (p[:blocks] >= 0).all() and (p[blocks:] == 0).all(), "a slot beyond the launched blocks was written"
    check_scalar(f"sumsq partials n={n} {dtype} off={offset}", p.double().sum(), ref)


@pytest.mark.parametrize("n", [0, 1, 257])
def test_reduce_sum_f32(n):
    ops = _ops()
    torch.manual_seed(n)
    x = torch.rand(n) + 0.5
    got = ops.reduce_sum_f32(x.to(DEV))
    assert got.shape == (1,) and got.dtype == torch.float32
    if n == 0:
        assert float(got) == 0.0
    else:
        check_scalar(f"reduce_sum_f32 n={n}", got, x.double().sum())


# ================================================================================================== 6. sumpool2
def sumpool2_ref(x):
    N, H2, W2, C = x.shape
    return x.float().view(N, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4)).to(BF)


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 3, 5, 24), (1, 64, 64, 320)])
def test_sumpool2_is_exact(shape):
    ops = _ops()
    N, H, W, C = shape
    torch.manual_seed(H * W)
    x = exact16(N, 2 * H, 2 * W, C)
    got = ops.sumpool2(x.to(DEV))
    assert got.shape == shape and torch.equal(got.cpu(), sumpool2_ref(x))


def test_sumpool2_behind_the_upsampling_conv():
    """ConvFn mode "up" with a 3x3 weight whose centre tap is a channel permutation: the forward is the nearest-2x upsampling of the
    permuted input and the input gradient is sumpool2 of the permuted upstream gradient, both exactly."""
    ops = _ops()
    torch.manual_seed(11)
    N, H, W, C = 2, 8, 8, 128
    perm = torch.randperm(C)
    Pm = torch.zeros(C, C)
    Pm[torch.arange(C), perm] = 1.0                          # y[co] = x[perm[co]]
    wf, wb = torch.zeros(C, 9, C), torch.zeros(C, 9, C)      # [CO, tap, CI] forward, flipped [CI, tap, CO] for the input gradient
    wf[:, 4], wb[:, 4] = Pm, Pm.t()
    x, dy = exact16(N, H, W, C), exact16(N, 2 * H, 2 * W, C)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.ConvFn.apply(xd, wf.view(C, -1).to(BF).to(DEV), wb.view(C, -1).to(BF).to(DEV), None, None, None, C, 3, "up")
    y.backward(dy.to(DEV))
    assert torch.equal(y.cpu(), x[..., perm].repeat_interleave(2, 1).repeat_interleave(2, 2))
    inv = torch.argsort(perm)
    assert torch.equal(xd.grad.cpu(), sumpool2_ref(dy)[..., inv])


# ================================================================================================== 7. row movers
@pytest.mark.parametrize("D", [8, 4096])
def test_scatter_rows_autograd(D):
    ops = _ops()
    torch.manual_seed(D)
    base, rows, dout = bf(2, 6, D), bf(3, D), bf(2, 6, D)
    idx = torch.tensor([7, 0, 11])
    bd, rd = base.to(DEV).requires_grad_(True), rows.to(DEV).requires_grad_(True)
    out = ops.scatter_rows(bd, idx.to(DEV), rd)
    out.backward(dout.to(DEV))
    ref = base.clone().view(-1, D)
    ref[idx] = rows
    assert torch.equal(out.cpu().view(-1, D), ref) and torch.equal(bd.detach().cpu(), base)
    dbase = dout.clone().view(-1, D)
    dbase[idx] = 0
    assert torch.equal(bd.grad.cpu().view(-1, D), dbase), "dbase must be zero at the spliced rows and dout elsewhere"
    assert torch.equal(rd.grad.cpu(), dout.view(-1, D)[idx]), "drows must be the gathered gradient"


@pytest.mark.parametrize("D", [8, 4096])
def test_gather_rows_autograd(D):
    ops = _ops()
    torch.manual_seed(D + 1)
    x, dout = bf(12, D), bf(5, D)
    idx = torch.tensor([9, 2, 11, 0, 5])
    xd = x.to(DEV).requires_grad_(True)
    out = ops.gather_rows_unique(xd, idx.to(DEV))
    out.backward(dout.to(DEV))
    assert torch.equal(out.cpu(), x[idx])
    dx = torch.zeros(12, D, dtype=BF)
    dx[idx] = dout
    assert torch.equal(xd.grad.cpu(), dx)


@pytest.mark.parametrize("D", [8, 4096])
def test_pack_and_unpack_rows_autograd(D):
    """tv = 5 valid tokens in 8 compact rows: the 3 filler rows repeat pad position 3, get no gradient, and pad positions of the
    unpacked grid come out zero"""
    ops = _ops()
    torch.manual_seed(D + 2)
    n_rows, tv = 12, 5
    idx = torch.tensor([9, 2, 11, 0, 5, 3, 3, 3])
    x, dout = bf(n_rows, D), bf(8, D)
    xd = x.to(DEV).requires_grad_(True)
    out = ops.PackRowsFn.apply(xd, idx.to(DEV), tv)
    out.backward(dout.to(DEV))
    assert torch.equal(out.cpu(), x[idx])
    dx = torch.zeros(n_rows, D, dtype=BF)
    dx[idx[:tv]] = dout[:tv]
    assert torch.equal(xd.grad.cpu(), dx), "filler rows must not send gradient to the pad position they repeat"

    rows, dgrid = bf(8, D), bf(n_rows, D)
    rd = rows.to(DEV).requires_grad_(True)
    grid = ops.UnpackRowsFn.apply(rd, idx.to(DEV), tv, n_rows)
    grid.backward(dgrid.to(DEV))
    ref = torch.zeros(n_rows, D, dtype=BF)
    ref[idx[:tv]] = rows[:tv]
    assert torch.equal(grid.cpu(), ref), "pad positions must come out zero"
    dr = torch.zeros(8, D, dtype=BF)
    dr[:tv] = dgrid[idx[:tv]]
    assert torch.equal(rd.grad.cpu(), dr)


@pytest.mark.parametrize("D", [8, 4096])
def test_gather_and_scatter_rows_layouts_and_index_types(D):
    ops = _ops()
    torch.manual_seed(D + 3)
    wide = bf(20, 2 * D)
    table = wide.to(DEV)[:, :D]                              # row-strided view: table.stride(0) = 2 D
    assert table.stride(0) > D
    idx = torch.tensor([[19, 0, 7], [7, 3, 19]])
    got = ops.gather_rows(table, idx.to(DEV))
    assert torch.equal(got.cpu(), wide[:, :D][idx.view(-1)])
    assert torch.equal(ops.gather_rows(table, idx.to(DEV).int()), got), "int32 indices must give the rows int64 ones give"

    src = bf(4, 2 * D)
    sidx = torch.tensor([5, 19, 0, 8])
    ref = wide.clone()
    ref[sidx, D:] = src[:, :D]
    for cast in (torch.int64, torch.int32):
        dst = wide.to(DEV)
        ops.scatter_rows_(dst[:, D:], sidx.to(DEV).to(cast), src.to(DEV)[:, :D])   # row-strided dst, row-strided src (copied)
        assert torch.equal(dst.cpu(), ref), f"scatter_rows_ with {cast} indices"


def test_gather_and_scatter_rows_reject_bad_layouts():
    ops = _ops()
    t = bf(16, 8).to(DEV)
    idx = torch.tensor([1, 2], device=DEV)
    with pytest.raises(ValueError):
        ops.gather_rows(t.t(), idx)                          # non-unit inner stride
    with pytest.raises(ValueError):
        ops.scatter_rows_(t.t(), idx, bf(2, 16).to(DEV))     # non-unit inner stride of dst
    with pytest.raises(ValueError):
        ops.scatter_rows_(t, idx, bf(2, 16).to(DEV))         # D differs between source and destination
    with pytest.raises(ValueError):
        ops.scatter_rows_(t, torch.tensor([1, 2, 3], device=DEV), bf(2, 8).to(DEV))   # more indices than source rows


# ================================================================================================== 8. GLU
GLU_VARIANTS = {"swiglu": (0, 1 << 62), "geglu": (1, 1 << 62), "swiglu_nt": (0, 0)}   # (mode, ops.GLU_NT_MIN_BYTES)


def glu_ref(mode, a, b, d):
    """float64 -> (out, da, db, floor of out, floor of da and db)"""
    a, b, d = f64(a), f64(b), f64(d)
    act, g = act_ref("silu" if mode == 0 else "gelu", a)
    fl = 2.0 ** -20 * a.abs().clamp_min(1.0) * b.abs().clamp_min(1.0)
    return act * b, d * b * g, d * act, fl, fl * d.abs().clamp_min(1.0)


@pytest.mark.parametrize("shape", [(3, 8),                   # one vector per row
                                   (5, 2056),                # 257 vectors: a second pass of the block with one live thread
                                   ((1 << 20) + 3, 8)])      # over the 2^20 cap of the row grid
@pytest.mark.parametrize("variant", list(GLU_VARIANTS))
def test_glu_fwd_bwd_match_float64(variant, shape):
    ops = _ops()
    mode, nt_min = GLU_VARIANTS[variant]
    M, F = shape
    torch.manual_seed(F)
    gu, d = bf(M, 2 * F, scale=2.0), bf(M, F)
    a, b = gu[:, :F], gu[:, F:]
    out_r, da_r, db_r, fl, fl_d = glu_ref(mode, a, b, d)
    gd, dd = gu.to(DEV), d.to(DEV)
    keep = ops.GLU_NT_MIN_BYTES
    ops.GLU_NT_MIN_BYTES = nt_min
    try:
        out = ops.glu_fwd(gd[:, :F], gd[:, F:], mode)
        da, db = ops.glu_bwd(dd, gd[:, :F], gd[:, F:], mode)
        dgu = torch.full((M, 2 * F), float("nan"), dtype=BF, device=DEV)    # da | db as the halves of one [M, 2F] buffer
        act = torch.empty(M, F, dtype=BF, device=DEV)
        da2, db2 = ops.glu_bwd(dd, gd[:, :F], gd[:, F:], mode, da=dgu[:, :F], db=dgu[:, F:], act_out=act)
    finally:
        ops.GLU_NT_MIN_BYTES = keep
    check_close(f"glu_fwd {variant} {shape}", out, out_r, fl)
    check_close(f"glu_bwd da {variant} {shape}", da, da_r, fl_d)
    check_close(f"glu_bwd db {variant} {shape}", db, db_r, fl_d)
    assert da2.data_ptr() == dgu.data_ptr() and torch.equal(dgu[:, :F], da) and torch.equal(dgu[:, F:], db)
    assert torch.equal(act, out), "act_out must be the forward product, bit for bit"


def test_glu_non_temporal_kernels_have_the_bits_of_the_plain_ones():
    ops = _ops()
    torch.manual_seed(12)
    M, F = 70, 352
    gu, d = bf(M, 2 * F, scale=2.0).to(DEV), bf(M, F).to(DEV)
    a, b = gu[:, :F], gu[:, F:]
    keep = ops.GLU_NT_MIN_BYTES
    res = {}
    try:
        for name, nt_min in (("plain", 1 << 62), ("nt", 0)):
            ops.GLU_NT_MIN_BYTES = nt_min
            assert ops._glu_mode(0, M, F) == (0x100 if name == "nt" else 0)
            act = torch.empty(M, F, dtype=BF, device=DEV)
            res[name] = (ops.glu_fwd(a, b, 0), *ops.glu_bwd(d, a, b, 0, act_out=act), act)
    finally:
        ops.GLU_NT_MIN_BYTES = keep
    for p, q in zip(res["plain"], res["nt"]):
        assert torch.equal(p, q)


# ================================================================================================== 9. softmax_rows
@pytest.mark.parametrize("cols", [4,        # one vector
                                  72,       # less than one pass of the block
                                  1028,     # between one and two passes
                                  4100])    # several passes plus a one-vector tail
def test_softmax_rows_matches_float64(cols):
    ops = _ops()
    torch.manual_seed(cols)
    x = torch.randn(6, cols) * 3.0
    x[1] += 80.0                            # exp overflows without the max subtraction
    x[2] -= 80.0                            # ... and underflows to 0 / 0
    x[3, cols // 3] = 60.0                  # one dominant entry
    x[4] = 1.25                             # a constant row
    x[5] = torch.randn(cols) * 20.0
    p = torch.softmax(x.double(), -1)
    got = ops.softmax_rows(x.to(DEV))
    assert got.dtype == BF and got.shape == x.shape
    check_close(f"softmax_rows cols={cols}", got, p, 2.0 ** -16)
    sums = f64(got).sum(-1)
    print(f"[elementwise] softmax_rows cols={cols}: row sums {sums.tolist()}")
    assert ((sums - 1.0).abs() <= 2.0 ** -7).all()
