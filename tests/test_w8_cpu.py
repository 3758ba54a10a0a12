"""CPU: FP8 weight-only decoding -- the quantiser's argument errors, `quantize_decode_weights`' format check (both come before any
device work) and the fp64 restatement the GPU tests rely on (tests/w8_ref.py) on hand-made rows."""
import pytest
import torch

from w8_ref import decode_e4m3, e4m3_table, gemv_w8_ref, quantize_rows_ref

BF = torch.bfloat16


def test_quantizer_argument_errors():
    from dreamllm_amd import ops
    with pytest.raises(ValueError):
        ops.quantize_rows_e4m3(torch.zeros(16, dtype=BF))               # not [N, K]
    with pytest.raises(ValueError):
        ops.quantize_rows_e4m3([[1.0, 2.0]])                            # not a tensor
    with pytest.raises(TypeError):
        ops.quantize_rows_e4m3(torch.zeros(4, 16))                      # fp32
    for bad in (float("inf"), float("-inf"), float("nan")):
        w = torch.ones(4, 16, dtype=BF)
        w[2, 5] = bad
        with pytest.raises(ValueError, match="finite"):
            ops.quantize_rows_e4m3(w)


def test_quantizer_rule_on_hand_made_rows():
    """The rule as `ops` states it equals the restatement, saturates, and treats zero / tiny / constant rows as the issue says."""
    from dreamllm_amd import ops
    torch.manual_seed(0)
    w = (torch.randn(6, 32) * 0.02).to(BF)
    w[1] = 0
    w[2] = 0
    w[2, 7] = 1e-30
    w[3] = -0.375
    q, s = ops.quantize_rows_e4m3(w)
    qr, sr = quantize_rows_ref(w)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and q.shape == w.shape and s.shape == (6,)
    assert torch.equal(q.view(torch.uint8), qr.view(torch.uint8)) and torch.equal(s, sr)
    v = decode_e4m3(q)
    assert not v.isnan().any()
    assert s[1] == 1 and (v[1] == 0).all()                              # an all-zero row: scale 1, zero codes
    assert v[2, 7] == 448 and (v[2, :7] == 0).all()                     # its only entry becomes the largest code
    assert (v[3] == -448).all() and s[3] == 0.375 / 448
    assert (v.abs().amax(1)[[0, 2, 3, 4, 5]] == 448).all()              # every non-zero row uses the whole range


def test_quantize_decode_weights_rejects_unknown_formats():
    from dreamllm_amd.factory import TINY, build_dreamllm
    lm = build_dreamllm(TINY, device="cpu", dtype=torch.float32, with_clip=False, with_sd=False).eval()
    for fmt in ("int4", "fp8_e5m2", "", 8):
        with pytest.raises(ValueError, match="format"):
            lm.quantize_decode_weights(fmt)
    assert lm.quantize_decode_weights(None) is None                     # dropping what was never set is fine


def test_w8_ops_reject_cpu_tensors():
    from dreamllm_amd import ops
    x = torch.zeros(1, 16, dtype=BF)
    q = torch.zeros(8, 16, dtype=torch.uint8).view(torch.float8_e4m3fn)
    s = torch.ones(8)
    with pytest.raises(RuntimeError):
        ops.gemv_w8(x, q, s)
    with pytest.raises(RuntimeError):
        ops.gemv_fused_w8(x, (q,), (s,))


def test_e4m3_table_against_torch():
    t = e4m3_table()
    codes = torch.arange(256, dtype=torch.uint8)
    tv = codes.view(torch.float8_e4m3fn).double()
    nan = torch.tensor([c in (0x7F, 0xFF) for c in range(256)])
    assert torch.equal(t.isnan(), nan) and torch.equal(tv.isnan(), nan)
    assert torch.equal(t[~nan], tv[~nan])
    assert t[0x7E] == 448 and t[0xFE] == -448 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0x38] == 1
    assert t[0x80] == 0 and torch.signbit(t[0x80])                      # -0 keeps its sign


def test_gemv_ref_on_hand_made_rows():
    """codes 0x38 = 1, 0x40 = 2, 0xC0 = -2, 0x30 = 0.5, 0x7E = 448."""
    q = torch.zeros(3, 16, dtype=torch.uint8)
    q[0, :4] = torch.tensor([0x38, 0x40, 0xC0, 0x30], dtype=torch.uint8)
    q[1, 15] = 0x7E
    scale = torch.tensor([0.5, 2.0, 3.0])
    x = torch.zeros(2, 16, dtype=BF)
    x[0, :4] = torch.tensor([1.0, 2.0, 3.0, 4.0]).to(BF)
    x[1, 15] = -1.0
    y, mag = gemv_w8_ref(x, q.view(torch.float8_e4m3fn), scale)
    assert y.dtype == torch.float64
    assert y.tolist() == [[0.5 * (1 + 4 - 6 + 2), 0.0, 0.0], [0.0, -896.0, 0.0]]
    assert mag.tolist() == [[0.5 * (1 + 4 + 6 + 2), 0.0, 0.0], [0.0, 896.0, 0.0]]
    r = torch.full((2, 3), 0.25, dtype=BF)
    y2, _ = gemv_w8_ref(x, q.view(torch.float8_e4m3fn), scale, residual=r)
    assert torch.equal(y2, y + 0.25)
