"""fp64 restatement of FP8 weight-only decoding (csrc/gemv_w8.hip, ops.quantize_rows_e4m3): the OCP e4m3fn code table decoded by
hand, the quantisation rule, and the GEMV  y[m][n] = scale[n] * sum_k q[n][k] * h[m][k] (+ residual[m][n]).  The GPU tests compare
the kernels against this file; tests/test_w8_cpu.py checks the file itself."""
import torch

E4M3_MAX = 448.0


def e4m3_table():
    """fp64 [256]: the value of every e4m3fn code -- sign, 4 exponent bits (bias 7), 3 mantissa bits, subnormals at exponent 0, no
    infinities, NaN at 0x7F / 0xFF."""
    vals = []
    for code in range(256):
        s, e, m = code >> 7, (code >> 3) & 15, code & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        vals.append(-v if s else v)
    return torch.tensor(vals, dtype=torch.float64)


def decode_e4m3(q):
    """float8_e4m3fn (or uint8 codes) -> fp64 values through the hand-made table."""
    codes = q.view(torch.uint8) if q.dtype != torch.uint8 else q
    return e4m3_table().to(codes.device)[codes.long()]


def quantize_rows_ref(w):
    """The quantisation rule, stated once: symmetric, one fp32 scale per output row, saturating at +-448."""
    wf = w.float()
    amax = wf.abs().amax(1)
    scale = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
    inv = 1 / scale
    q = (wf * inv[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q, scale


def gemv_w8_ref(x, q, scale, residual=None):
    """-> (y, mag) fp64 [M, N]: y = scale[n] * sum_k q[n][k] x[m][k] (+ residual), mag = scale[n] * sum_k |q[n][k] x[m][k]| (the
    magnitude the accumulation-error bound of the GPU test scales with)."""
    qd, xd, sd = decode_e4m3(q), x.double(), scale.double()
    y = (xd @ qd.t()) * sd[None, :]
    mag = (xd.abs() @ qd.abs().t()) * sd[None, :]
    if residual is not None:
        y = y + residual.double()
    return y, mag
