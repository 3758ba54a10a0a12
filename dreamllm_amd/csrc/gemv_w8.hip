// FP8 weight-only decode GEMVs for gfx950: the batch-1..8 Linear of the token step with the weight stored as OCP e4m3fn codes
// (one byte per element, symmetric, one fp32 scale per output row; ops.quantize_rows_e4m3) -- half the bytes of csrc/decode.hip's
// bf16 family on the stream that bounds the step.
//
//   y[m][n] = round_out( scale[n] * sum_k q[n][k] * h[m][k]  (+ residual[m][n]) ),   h = x  or  bf16(norm_w * bf16(x * rstd))
//
// Every e4m3 value is exact in bf16, so a code pair is converted in one instruction (v_cvt_scalef32_pk_bf16_fp8, scale 1) and
// multiplied with v_dot2c_f32_bf16 like the bf16 kernel: 8 conversions + 8 * M dot2 per 16 weight bytes, fp32 accumulation.  The
// scale multiplies the wave-reduced sum once, before the residual add and the output rounding.
//
// One kernel, modelled on gemv_lds_kernel: a wave owns R = 2 consecutive output rows per row set, a lane 16 codes (one 16-byte
// non-temporal load) of each 1024-element chunk, U = 4 chunks per batch, two register sets in flight, both requested before x is
// touched.  x comes from one of two places (template XLDS), chosen from (M, K) alone so that a plain and a fused call over the same
// operands run the same form and accumulate in the same order:
//   * XLDS: staged once per block in LDS, already normalised (wave 0 computes rstd in rmsnorm_fwd_kernel's lane / vector order).  A
//     lane multiplies its 16 codes with 32 bytes of x; stored in k order that is a 32-byte lane stride (2-way bank conflict on
//     ds_read_b128), so every 1024-element chunk is stored as the 64 lanes' first 8 elements, then their second 8: both reads are
//     lane * 16 bytes.
//   * otherwise (M > 4, or x larger than the LDS budget: M = 8 with K = 11008): read from L1 / L2 per wave and normalised on the
//     fly with the same two roundings, rstd recomputed by every wave in the same order (gemv_fused_kernel's way).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;

struct GemvW8Params {
    const bf16* x;          // [M][ldx]
    const bf16* norm_w;     // [K] or null
    float eps;
    const uint8_t* W[3];    // e4m3fn codes [N_i][ldw]
    const float* scale[3];  // [N_i]
    void* y[3];             // [M][ldy_i]
    int64_t N[3];
    int64_t ldy[3];
    const bf16* residual;   // added to y[0] or null
    int64_t ldr;
    int K;
    int64_t ldx, ldw;
    int out_f32;
};

struct Bf16x8Pairs {
    bf16x2v p[4];
};

// 16 codes -> 8 bf16 pairs in k order (exact: e4m3 has 3 mantissa bits)
__device__ __forceinline__ void dequant16(const u32x4& c, bf16x2v (&w)[8]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        w[2 * d] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[d], 1.0f, false);
        w[2 * d + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[d], 1.0f, true);
    }
}

// the ONE accumulation order of the family: the lane's 16 products of a chunk, pair by pair in k order
__device__ __forceinline__ float dot16(const bf16x2v (&w)[8], const bf16x8& xlo, const bf16x8& xhi, float acc) {
    const Bf16x8Pairs lo = __builtin_bit_cast(Bf16x8Pairs, xlo), hi = __builtin_bit_cast(Bf16x8Pairs, xhi);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_fdot2_f32_bf16(w[e], lo.p[e], acc, false);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_fdot2_f32_bf16(w[4 + e], hi.p[e], acc, false);
    return acc;
}

// scale[n] * sum as ONE rounded product: it must not contract with the residual add that follows
__device__ __forceinline__ float scaled(float sum, float s) {
#pragma clang fp reassociate(off) contract(off)
    return sum * s;
}

__device__ __forceinline__ bf16x8 rmsnorm8(bf16x8 xv, const bf16x8& nw, float rs) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bf16 t = (bf16)((float)xv[e] * rs);   // .to(input_dtype)
        xv[e] = (bf16)((float)nw[e] * (float)t);    // weight * (.)
    }
    return xv;
}

static inline int w8_kpad(int64_t K) { return (int)((K + 1023) / 1024 * 1024); }

template <int MB, bool SWIGLU, bool XLDS>
__global__ __launch_bounds__(256) void gemv_w8_kernel(GemvW8Params P, int iters) {
    constexpr int R = 2, U = 4;               // rows per wave and row set, 1024-element chunks per batch
    constexpr int NW = SWIGLU ? 2 : 1;        // weight streams per row (gate, up)
    constexpr int STEP = 1024 * U;
    constexpr int MG = MB < 4 ? MB : 4;       // x rows held in registers at a time
    extern __shared__ __attribute__((aligned(16))) char smem_w8[];
    bf16* xs = reinterpret_cast<bf16*>(smem_w8);   // XLDS: [MB][kpad], chunk-permuted (see the head of the file)
    __shared__ float rstd_s[MB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = P.K;
    const int kpad = (K + 1023) / 1024 * 1024;
    const int64_t total_rows = SWIGLU ? P.N[0] : P.N[0] + P.N[1] + P.N[2];
    // a wave owns `iters` consecutive row sets of R rows; its work is the flat sequence of (row set, K batch) pairs
    const int64_t set0 = ((int64_t)blockIdx.x * 4 + wave) * iters;
    const int nbk = (K + STEP - 1) / STEP;
    const int total = iters * nbk;
    // (matrix, row inside it, live) of row r of row set `it`
    auto row_desc = [&](int it, int r, int& mt, int64_t& n, bool& lv) {
        n = (set0 + it) * R + r;
        lv = n < total_rows;
        if (!lv) n = total_rows - 1;          // a valid row: loaded, never stored
        mt = 0;
        if constexpr (!SWIGLU) {
            if (n >= P.N[0]) {
                n -= P.N[0];
                mt = 1;
                if (n >= P.N[1]) {
                    n -= P.N[1];
                    mt = 2;
                }
            }
        }
    };
    auto load_batch = [&](u32x4 (&dst)[R][NW][U], int j) {
        const int it = j / nbk, k0 = (j - it * nbk) * STEP;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int mt;
            int64_t n;
            bool lv;
            row_desc(it, r, mt, n, lv);
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                const uint8_t* wr = (SWIGLU ? P.W[q] : P.W[mt]) + n * P.ldw;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * 1024 + lane * 16;
                    const u32x4 z = {0u, 0u, 0u, 0u};
                    dst[r][q][u] = k < K ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + k)) : z;
                }
            }
        }
    };
    u32x4 wa[R][NW][U], wb[R][NW][U];
    load_batch(wa, 0);   // both register sets are requested before x is touched: the weights do not depend on it
    if (total > 1) load_batch(wb, 1);

    // ---- rstd: wave 0 for the block (XLDS) or every wave for itself, in rmsnorm_fwd_kernel's lane / vector order ----------------
    float rstd[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) rstd[m] = 0.f;
    if (P.norm_w != nullptr) {
        if (!XLDS || wave == 0) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                float ss = 0.f;
                for (int k = lane * 8; k < K; k += 512) {
                    const bf16x8 xv = ld_bf16x8(P.x + m * P.ldx + k);
#pragma unroll
                    for (int e = 0; e < 8; ++e) ss += (float)xv[e] * (float)xv[e];
                }
                ss = wave_sum(ss);
                rstd[m] = rsqrtf(ss / (float)K + P.eps);
                if (XLDS && lane == 0) rstd_s[m] = rstd[m];
            }
        }
    }
    if constexpr (XLDS) {
        if (P.norm_w != nullptr) __syncthreads();
        // x -> LDS, normalised when norm_w is given: 8-element group g of chunk c goes to group (g & 1) * 64 + (g >> 1) of the chunk
        for (int g = threadIdx.x; g < (K >> 3); g += 256) {
            const int k = g * 8, gc = g & 127;
            const int dst = (g >> 7) * 1024 + ((gc & 1) * 64 + (gc >> 1)) * 8;
            bf16x8 nw = zero_bf16x8();
            if (P.norm_w != nullptr) nw = ld_bf16x8(P.norm_w + k);
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                bf16x8 xv = ld_bf16x8(P.x + m * P.ldx + k);
                if (P.norm_w != nullptr) xv = rmsnorm8(xv, nw, rstd_s[m]);
                *reinterpret_cast<bf16x8*>(xs + (int64_t)m * kpad + dst) = xv;
            }
        }
        __syncthreads();
    }

    float acc[R][NW][MB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < NW; ++q)
#pragma unroll
            for (int m = 0; m < MB; ++m) acc[r][q][m] = 0.f;
    // batch j: accumulate; after the last batch of a row set reduce over the wave, store its R rows, clear the accumulators
    auto consume = [&](const u32x4 (&src)[R][NW][U], int j) {
        const int it = j / nbk, kb = j - it * nbk, k0 = kb * STEP;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kc = k0 + u * 1024, k = kc + lane * 16;
            if (k < K) {
                bf16x8 nlo = zero_bf16x8(), nhi = zero_bf16x8();
                if constexpr (!XLDS) {
                    if (P.norm_w != nullptr) {
                        nlo = ld_bf16x8(P.norm_w + k);
                        nhi = ld_bf16x8(P.norm_w + k + 8);
                    }
                }
#pragma unroll
                for (int m0 = 0; m0 < MB; m0 += MG) {
                    bf16x8 xlo[MG], xhi[MG];
#pragma unroll
                    for (int mm = 0; mm < MG; ++mm) {
                        const int m = m0 + mm;
                        if (m < MB) {
                            if constexpr (XLDS) {
                                const bf16* xp = xs + (int64_t)m * kpad + kc + lane * 8;
                                xlo[mm] = *reinterpret_cast<const bf16x8*>(xp);
                                xhi[mm] = *reinterpret_cast<const bf16x8*>(xp + 512);
                            } else {
                                xlo[mm] = ld_bf16x8(P.x + m * P.ldx + k);
                                xhi[mm] = ld_bf16x8(P.x + m * P.ldx + k + 8);
                                if (P.norm_w != nullptr) {
                                    xlo[mm] = rmsnorm8(xlo[mm], nlo, rstd[m]);
                                    xhi[mm] = rmsnorm8(xhi[mm], nhi, rstd[m]);
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int q = 0; q < NW; ++q) {
                            bf16x2v w[8];
                            dequant16(src[r][q][u], w);
#pragma unroll
                            for (int mm = 0; mm < MG; ++mm)
                                if (m0 + mm < MB) acc[r][q][m0 + mm] = dot16(w, xlo[mm], xhi[mm], acc[r][q][m0 + mm]);
                        }
                }
            }
        }
        if (kb != nbk - 1) return;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int mt;
            int64_t n;
            bool lv;
            row_desc(it, r, mt, n, lv);
            const float s0 = SWIGLU ? P.scale[0][n] : P.scale[mt][n];
            float s1 = 0.f;
            if constexpr (SWIGLU) s1 = P.scale[1][n];
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const float v = scaled(wave_sum(acc[r][0][m]), s0);
                float v1 = 0.f;
                if constexpr (SWIGLU) v1 = scaled(wave_sum(acc[r][1][m]), s1);
                acc[r][0][m] = 0.f;
                if constexpr (SWIGLU) acc[r][1][m] = 0.f;
                if (lane == 0 && lv) {
                    if constexpr (SWIGLU) {
                        const float g = (float)(bf16)v, u_ = (float)(bf16)v1;
                        reinterpret_cast<bf16*>(P.y[0])[m * P.ldy[0] + n] = (bf16)swiglu_fwd_elem(g, u_);
                    } else {
                        float o = v;
                        if (P.residual != nullptr && mt == 0) o += (float)P.residual[m * P.ldr + n];
                        if (P.out_f32)
                            reinterpret_cast<float*>(P.y[mt])[m * P.ldy[mt] + n] = o;
                        else
                            reinterpret_cast<bf16*>(P.y[mt])[m * P.ldy[mt] + n] = (bf16)o;
                    }
                }
            }
        }
    };
    for (int j = 0; j < total; j += 2) {
        consume(wa, j);
        if (j + 2 < total) load_batch(wa, j + 2);
        if (j + 1 < total) {
            consume(wb, j + 1);
            if (j + 3 < total) load_batch(wb, j + 3);
        }
    }
}

// LDS-staged x: M <= 4 rows of kpad bf16 inside the default 64 KiB of dynamic LDS (the bf16 family's rule, on the padded K)
static inline bool w8_lds_ok(int M, int64_t K) { return M <= 4 && (int64_t)M * w8_kpad(K) * 2 <= 60 * 1024; }

template <int MB>
int launch_gemv_w8(const GemvW8Params& P, int swiglu, hipStream_t s) {
    const int64_t rows = swiglu ? P.N[0] : P.N[0] + P.N[1] + P.N[2];
    // row sets per wave: as few as keep the grid inside one resident round (launch_gemv_lds' rule; resident blocks per CU from this
    // kernel's registers at batch 1: 98 per lane, 162 with two weight streams)
    const int64_t slots = (int64_t)dllm_num_cus() * (swiglu ? 3 : 4);
    int iters = (int)cdiv64(cdiv64(rows, 8), slots);
    iters = iters < 1 ? 1 : (iters > 4 ? 4 : iters);
    const unsigned grid = (unsigned)cdiv64(rows, 8 * (int64_t)iters);
    if constexpr (MB <= 4) {
        if (w8_lds_ok(MB, P.K)) {
            const size_t lds = (size_t)MB * w8_kpad(P.K) * 2;
            if (swiglu)
                hipLaunchKernelGGL((gemv_w8_kernel<MB, true, true>), dim3(grid), dim3(256), lds, s, P, iters);
            else
                hipLaunchKernelGGL((gemv_w8_kernel<MB, false, true>), dim3(grid), dim3(256), lds, s, P, iters);
            return dllm_check_launch();
        }
    }
    if (swiglu)
        hipLaunchKernelGGL((gemv_w8_kernel<MB, true, false>), dim3(grid), dim3(256), 0, s, P, iters);
    else
        hipLaunchKernelGGL((gemv_w8_kernel<MB, false, false>), dim3(grid), dim3(256), 0, s, P, iters);
    return dllm_check_launch();
}

int dispatch_gemv_w8(const GemvW8Params& P, int M, int swiglu, hipStream_t s) {
    switch (M) {
        case 1: return launch_gemv_w8<1>(P, swiglu, s);
        case 2: return launch_gemv_w8<2>(P, swiglu, s);
        case 3: return launch_gemv_w8<3>(P, swiglu, s);
        case 4: return launch_gemv_w8<4>(P, swiglu, s);
        case 5: return launch_gemv_w8<5>(P, swiglu, s);
        case 6: return launch_gemv_w8<6>(P, swiglu, s);
        case 7: return launch_gemv_w8<7>(P, swiglu, s);
        default: return launch_gemv_w8<8>(P, swiglu, s);
    }
}

inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" {

// y[M][N] = scale[n] * (x[M][K] Q[N][K]^T) (+ residual[M][N]); M <= 8, K % 16 == 0; x bf16, Q e4m3fn codes (ldw in bytes), scale fp32
// [N]; fp32 accumulation; out_dtype DLLM_BF16 / DLLM_F32.  The FP8 weight-only twin of dllm_gemv_bf16.
int dllm_gemv_w8(const void* x, const void* Wq, const float* scale, void* y, const void* residual, int M, int64_t N, int64_t K,
                 int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, int out_dtype, void* stream) {
    if (M < 0 || M > 8 || N < 0 || K <= 0 || K > 0x7fffffff || (K & 15)) return DLLM_ERR_SHAPE;
    if (x == nullptr || Wq == nullptr || scale == nullptr || y == nullptr) return DLLM_ERR_SHAPE;
    if ((ldx & 7) || (ldw & 15) || misaligned16(x) || misaligned16(Wq)) return DLLM_ERR_ALIGN;
    if (out_dtype != DLLM_BF16 && out_dtype != DLLM_F32) return DLLM_ERR_DTYPE;
    if (M == 0 || N == 0) return DLLM_OK;
    GemvW8Params P{};
    P.x = (const bf16*)x; P.W[0] = (const uint8_t*)Wq; P.scale[0] = scale; P.y[0] = y; P.N[0] = N; P.ldy[0] = ldy;
    P.residual = (const bf16*)residual; P.ldr = ldr; P.K = (int)K; P.ldx = ldx; P.ldw = ldw; P.out_f32 = out_dtype == DLLM_F32;
    return dispatch_gemv_w8(P, M, 0, (hipStream_t)stream);
}

// The FP8 weight-only twin of dllm_gemv_fused: h = RMSNorm(x; norm_w, eps) if norm_w else x; y_i = scale_i * (h Q_i^T) for up to
// three matrices sharing K and ldw (q|k|v), optional residual added to y_0; swiglu != 0: (gate, up) ->
// y_0 = bf16(silu(bf16(s_g acc_g)) * bf16(s_u acc_u)).
int dllm_gemv_fused_w8(const void* x, const void* norm_w, float eps, const void* W0, const void* W1, const void* W2, const float* s0,
                       const float* s1, const float* s2, void* y0, void* y1, void* y2, const void* residual, int M, int64_t N0,
                       int64_t N1, int64_t N2, int64_t K, int64_t ldx, int64_t ldw, int64_t ldy0, int64_t ldy1, int64_t ldy2,
                       int64_t ldr, int swiglu, int out_dtype, void* stream) {
    if (M < 0 || M > 8 || N0 < 0 || N1 < 0 || N2 < 0 || K <= 0 || K > 0x7fffffff || (K & 15)) return DLLM_ERR_SHAPE;
    if (x == nullptr || W0 == nullptr || s0 == nullptr || y0 == nullptr) return DLLM_ERR_SHAPE;
    if (swiglu && (W1 == nullptr || s1 == nullptr || N1 != N0 || N2 != 0 || out_dtype != DLLM_BF16 || residual != nullptr))
        return DLLM_ERR_SHAPE;
    if ((N1 > 0 && (W1 == nullptr || s1 == nullptr || (!swiglu && y1 == nullptr))) ||
        (N2 > 0 && (W2 == nullptr || s2 == nullptr || y2 == nullptr)))
        return DLLM_ERR_SHAPE;
    if ((ldx & 7) || (ldw & 15) || misaligned16(x) || misaligned16(W0) || (N1 > 0 && misaligned16(W1)) ||
        (N2 > 0 && misaligned16(W2)) || (norm_w != nullptr && misaligned16(norm_w)))
        return DLLM_ERR_ALIGN;
    if (out_dtype != DLLM_BF16 && out_dtype != DLLM_F32) return DLLM_ERR_DTYPE;
    if (M == 0 || N0 == 0) return DLLM_OK;
    GemvW8Params P{};
    P.x = (const bf16*)x; P.norm_w = (const bf16*)norm_w; P.eps = eps;
    P.W[0] = (const uint8_t*)W0; P.W[1] = (const uint8_t*)W1; P.W[2] = (const uint8_t*)W2;
    P.scale[0] = s0; P.scale[1] = s1; P.scale[2] = s2;
    P.y[0] = y0; P.y[1] = y1; P.y[2] = y2;
    P.N[0] = N0; P.N[1] = swiglu ? N0 : N1; P.N[2] = N2;
    P.ldy[0] = ldy0; P.ldy[1] = ldy1; P.ldy[2] = ldy2;
    P.residual = (const bf16*)residual; P.ldr = ldr; P.K = (int)K; P.ldx = ldx; P.ldw = ldw; P.out_f32 = out_dtype == DLLM_F32;
    return dispatch_gemv_w8(P, M, swiglu, (hipStream_t)stream);
}

}  // extern "C"
