// CLIP text-image scoring: the pooled tail of both CLIP towers and the best-of-N selection of the reference's text-to-image
// evaluation, two launches in all.  This is what `HipCLIPModel.forward()` / `.select()` and `DreamLLMForCausalMLM.best_of_n()` run
// above the towers' GEMM / attention kernels.
//
// Reference call sites: omni/eval/text2img/ddp_sample_coco.py `select_image` (transformers `CLIPModel(**inputs).logits_per_image`,
// `argmax(logits_per_image) // logits_per_image.shape[1]` over the eight images sampled for one caption set); transformers 4.35.2 [ext]
// modeling_clip.py `CLIPModel.forward` (pooled_output -> final / post LayerNorm -> projection without bias -> x / ||x|| ->
// exp(logit_scale) * text_embeds @ image_embeds.T).
//
// ---- dllm_clip_embed_head: pooled row -> LayerNorm -> projection -> L2 normalise, one block of 256 threads per row b
//   r     = pos == NULL ? 0 : clamp(pos[b], 0, S - 1)           (NULL: the vision tower's CLS token; device data never leaves the row)
//   x_k   = fp32(hidden[b, r, k])                                (bf16 [B, S, H], element strides sb / ss, H contiguous)
//   mean  = (1 / H) sum_k x_k,  var = (1 / H) sum_k (x_k - mean)^2   (two passes over the registers, fp32)
//   y_k   = (x_k - mean) * rsqrt(var + eps) * w_k + b_k          (kept in fp32: NOT rounded to bf16, unlike the towers' LayerNorm kernel)
//   e_p   = sum_k proj[p, k] * y_k                               (proj bf16 [P, H], no bias; fp32 accumulation)
//   raw[b, p] = e_p (optional: what get_*_features returns);  embeds[b, p] = e_p / sqrt(sum_p e_p^2)
//   sum_p e_p^2 zero, NaN or infinite: embeds[b, :] = 0 and status[b] = 1 (status is optional and only ever set, never cleared)
// Form: thread t holds the 8 values of 16-byte vector t of the row (H <= 2048 = 256 x 8); the two block sums go butterfly -> the wave
// totals added in wave order; y is staged in LDS and re-read so that in EVERY wave lane l holds vectors l, l + 64, ... of y in
// registers; the waves take the output columns strided (wave w: p = w, w + 4, ...), four columns per trip so that up to 16
// 16-byte loads of `proj` are in flight, each column's partial sums finished by a butterfly (every lane ends with the same bits).
// The un-normalised e goes to `embeds` first; after the block barrier all 256 threads rescale it in place (coalesced).
// The squared norm is each wave's running sum over ITS columns in ascending order, then the four wave sums in wave order.
//
// ---- dllm_clip_select: scaled similarities and the reference's selection rule for G groups, one block of 256 threads per group g
//   images  i in [img_start[g], img_start[g + 1]) (n of them), texts j in [txt_start[g], txt_start[g + 1]) (m of them); int32 [G + 1]
//   logit(i, j) = scale * sum_d img[i, d] * txt[j, d]            (fp32 unit rows [NI, D] / [NT, D]; NOT renormalised here)
//   logits[out_start[g] + i * m + j] = logit(i, j)               (optional; group g row-major [n, m], out_start[g] = sum of earlier n * m)
//   best[g]       = (the lowest flat index i * m + j of the largest FINITE logit) / m       (torch.argmax's first occurrence, // m)
//   best_logit[g] = that logit
//   a NaN or an infinity among the group's logits ranks below every finite one and sets status[g] = 1; a group without a finite logit
//   (or, from bad device data only, without an image or a text) returns best 0, best_logit NaN, status 1.  The start arrays are device
//   data: spans are clamped to [0, NI] / [0, NT], and a group whose logits would not fit [0, n_logits) writes none and sets status 2.
// Form: a wave per (i, j) pair, strided (wave w: flat index w, w + 4, ...: ascending, so `>` keeps the first occurrence); lanes
// stride over D with 16-byte loads and finish with a butterfly; each wave keeps (value, flat index) of its best; thread 0 merges the
// four wave bests in wave order (larger value, then lower index).
//
// Both: plain vector loads and stores, wave butterflies, LDS; no float atomics, every float sum has a fixed order -> the same
// inputs give the same bits on every launch.  -0.0 and +0.0 are equal, as in every float comparison.
#include "common.h"

namespace {

constexpr int CLIP_THREADS = 256;
constexpr int CLIP_NW = CLIP_THREADS / 64;
constexpr int CLIP_MAX_H = 2048;              // one 16-byte vector of the row per thread
constexpr int CLIP_NI = CLIP_MAX_H / 8 / 64;  // vectors of y per lane
constexpr int CLIP_COLS = 4;                  // output columns per wave and trip

__device__ __forceinline__ float dot8(bf16x8 w, const float* y, float acc) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(bf2f(w[e]), y[e], acc);
    return acc;
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_embed_head_kernel(const bf16* __restrict__ hidden, int64_t sb, int64_t ss, int S, int H,
                                                                       const int64_t* __restrict__ pos, const bf16* __restrict__ ln_w,
                                                                       const bf16* __restrict__ ln_b, float eps, const bf16* __restrict__ proj,
                                                                       int P, float* __restrict__ embeds, float* __restrict__ raw,
                                                                       int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float s_y[CLIP_MAX_H];
    __shared__ float s_red[CLIP_NW];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nvec = H >> 3;
    int64_t r = 0;
    if (pos != nullptr) {
        r = pos[b];
        r = r < 0 ? 0 : (r > S - 1 ? S - 1 : r);
    }
    const bf16* row = hidden + b * sb + r * ss;

    // ---- LayerNorm of the pooled row, two passes over the registers
    const bool own = tid < nvec;
    float x[8];
    float sum = 0.f;
    if (own) {
        const bf16x8 v = ld_bf16x8(row + tid * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] = bf2f(v[e]);
            sum += x[e];
        }
    }
    const float mean = block_sum<CLIP_NW>(sum, s_red) / (float)H;
    float sq = 0.f;
    if (own) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = x[e] - mean;
            sq += d * d;
        }
    }
    const float rstd = 1.0f / sqrtf(block_sum<CLIP_NW>(sq, s_red) / (float)H + eps);
    if (own) {
        const bf16x8 gw = ld_bf16x8(ln_w + tid * 8), gb = ld_bf16x8(ln_b + tid * 8);
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo[e] = (x[e] - mean) * rstd * bf2f(gw[e]) + bf2f(gb[e]);
            hi[e] = (x[e + 4] - mean) * rstd * bf2f(gw[e + 4]) + bf2f(gb[e + 4]);
        }
        *reinterpret_cast<f32x4*>(&s_y[tid * 8]) = lo;
        *reinterpret_cast<f32x4*>(&s_y[tid * 8 + 4]) = hi;
    }
    __syncthreads();

    // ---- every wave: lane l takes vectors l, l + 64, ... of y into registers
    float y[CLIP_NI][8];
#pragma unroll
    for (int i = 0; i < CLIP_NI; ++i) {
        const int c = lane + i * 64;
        if (c < nvec) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(&s_y[c * 8]);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(&s_y[c * 8 + 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[i][e] = lo[e];
                y[i][e + 4] = hi[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) y[i][e] = 0.f;
        }
    }

    // ---- projection: wave w takes columns w, w + 4, ..., CLIP_COLS of them per trip
    float* erow = embeds + b * (int64_t)P;
    float* rrow = raw != nullptr ? raw + b * (int64_t)P : nullptr;
    float ssq = 0.f;
    for (int p0 = w; p0 < P; p0 += CLIP_NW * CLIP_COLS) {
        bf16x8 wv[CLIP_COLS][CLIP_NI];
#pragma unroll
        for (int j = 0; j < CLIP_COLS; ++j) {
            const int p = p0 + j * CLIP_NW;
#pragma unroll
            for (int i = 0; i < CLIP_NI; ++i) {
                const int c = lane + i * 64;
                wv[j][i] = (p < P && c < nvec) ? ld_bf16x8(proj + (int64_t)p * H + c * 8) : zero_bf16x8();
            }
        }
#pragma unroll
        for (int j = 0; j < CLIP_COLS; ++j) {
            const int p = p0 + j * CLIP_NW;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < CLIP_NI; ++i) acc = dot8(wv[j][i], y[i], acc);
            acc = wave_sum(acc);
            if (p < P) {
                ssq += acc * acc;
                if (lane == 0) {
                    erow[p] = acc;
                    if (rrow != nullptr) rrow[p] = acc;
                }
            }
        }
    }
    __syncthreads();  // s_red is free again (block_sum's last reads are behind the barrier above); erow is visible to the block after the next one
    if (lane == 0) s_red[w] = ssq;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < CLIP_NW; ++i) total += s_red[i];
    const float norm = sqrtf(total);
    const bool ok = norm > 0.f && norm < INFINITY;
    for (int p = tid; p < P; p += CLIP_THREADS) erow[p] = ok ? erow[p] / norm : 0.f;
    if (!ok && tid == 0 && status != nullptr) status[b] = 1;
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_select_kernel(const float* __restrict__ img, const float* __restrict__ txt, int NI, int NT,
                                                                   int D, const int* __restrict__ img_start, const int* __restrict__ txt_start,
                                                                   const int* __restrict__ out_start, float scale, float* __restrict__ logits,
                                                                   int64_t n_logits, int64_t* __restrict__ best, float* __restrict__ best_logit,
                                                                   int* __restrict__ status) {
    __shared__ float s_val[CLIP_NW];
    __shared__ int s_idx[CLIP_NW], s_bad[CLIP_NW];
    const int g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int i0 = img_start[g], i1 = img_start[g + 1], j0 = txt_start[g], j1 = txt_start[g + 1];
    i0 = i0 < 0 ? 0 : (i0 > NI ? NI : i0);  // device data: stay inside the arrays whatever it holds
    i1 = i1 < i0 ? i0 : (i1 > NI ? NI : i1);
    j0 = j0 < 0 ? 0 : (j0 > NT ? NT : j0);
    j1 = j1 < j0 ? j0 : (j1 > NT ? NT : j1);
    const int n = i1 - i0, m = j1 - j0;
    const int64_t pairs = (int64_t)n * m;
    const int64_t o0 = out_start[g];
    const bool fits = o0 >= 0 && o0 <= n_logits && pairs <= n_logits - o0;
    float* out = (logits != nullptr && fits) ? logits + o0 : nullptr;
    const int nvec = D >> 2;

    float bv = 0.f;
    int bi = -1;  // no finite logit yet
    int bad = 0;
    for (int64_t q = w; q < pairs; q += CLIP_NW) {
        const int i = (int)(q / m), j = (int)(q - (int64_t)i * m);
        const float* a = img + (int64_t)(i0 + i) * D;
        const float* t = txt + (int64_t)(j0 + j) * D;
        float acc = 0.f;
        for (int c = lane; c < nvec; c += 64) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(a + c * 4);
            const f32x4 tv = *reinterpret_cast<const f32x4*>(t + c * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(av[e], tv[e], acc);
        }
        const float lg = scale * wave_sum(acc);
        if (out != nullptr && lane == 0) out[q] = lg;
        const bool fin = lg > -INFINITY && lg < INFINITY;  // false for a NaN
        if (!fin) bad = 1;
        else if (bi < 0 || lg > bv) {
            bv = lg;
            bi = (int)q;
        }
    }
    if (lane == 0) {
        s_val[w] = bv;
        s_idx[w] = bi;
        s_bad[w] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        float v = 0.f;
        int idx = -1, anybad = 0;
#pragma unroll
        for (int k = 0; k < CLIP_NW; ++k) {
            anybad |= s_bad[k];
            const int ik = s_idx[k];
            const float vk = s_val[k];
            if (ik >= 0 && (idx < 0 || vk > v || (vk == v && ik < idx))) {
                v = vk;
                idx = ik;
            }
        }
        best[g] = idx < 0 ? 0 : (int64_t)(idx / m);
        best_logit[g] = idx < 0 ? __uint_as_float(0x7FC00000u) : v;
        const int st = ((anybad || idx < 0) ? 1 : 0) | ((logits != nullptr && !fits) ? 2 : 0);
        if (st != 0 && status != nullptr) status[g] |= st;
    }
}

}  // namespace

extern "C" int dllm_clip_embed_head(const void* hidden, int64_t sb, int64_t ss, int B, int S, int H, const int64_t* pos, const void* ln_w,
                                    const void* ln_b, float eps, const void* proj, int P, float* embeds, float* raw, int* status,
                                    void* stream) {
    if (B < 0 || S < 1 || H < 8 || (H & 7) || H > CLIP_MAX_H || P < 1 || P > (1 << 24) || sb < 0 || ss < 0) return DLLM_ERR_SHAPE;
    if (B == 0) return DLLM_OK;
    if (hidden == nullptr || ln_w == nullptr || ln_b == nullptr || proj == nullptr || embeds == nullptr) return DLLM_ERR_SHAPE;
    if ((sb & 7) || (ss & 7)) return DLLM_ERR_ALIGN;
    if ((reinterpret_cast<uintptr_t>(hidden) | reinterpret_cast<uintptr_t>(ln_w) | reinterpret_cast<uintptr_t>(ln_b) |
         reinterpret_cast<uintptr_t>(proj)) & 15)
        return DLLM_ERR_ALIGN;
    hipLaunchKernelGGL(clip_embed_head_kernel, dim3((unsigned)B), dim3(CLIP_THREADS), 0, (hipStream_t)stream, static_cast<const bf16*>(hidden),
                       sb, ss, S, H, pos, static_cast<const bf16*>(ln_w), static_cast<const bf16*>(ln_b), eps, static_cast<const bf16*>(proj), P,
                       embeds, raw, status);
    return dllm_check_launch();
}

extern "C" int dllm_clip_select(const float* img, const float* txt, int NI, int NT, int D, int G, const int* img_start, const int* txt_start,
                                const int* out_start, float scale, float* logits, int64_t n_logits, int64_t* best, float* best_logit,
                                int* status, void* stream) {
    if (G < 0 || NI < 0 || NT < 0 || D < 4 || (D & 3) || n_logits < 0 || (int64_t)NI * NT > 0x7FFFFFFF) return DLLM_ERR_SHAPE;
    if (G == 0) return DLLM_OK;
    if (img == nullptr || txt == nullptr || img_start == nullptr || txt_start == nullptr || out_start == nullptr || best == nullptr ||
        best_logit == nullptr)
        return DLLM_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(txt)) & 15) return DLLM_ERR_ALIGN;
    hipLaunchKernelGGL(clip_select_kernel, dim3((unsigned)G), dim3(CLIP_THREADS), 0, (hipStream_t)stream, img, txt, NI, NT, D, img_start,
                       txt_start, out_start, scale, logits, n_logits, best, best_logit, status);
    return dllm_check_launch();
}
