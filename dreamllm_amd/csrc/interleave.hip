// Device-side pieces of interleaved text-and-image generation (`generate_interleaved`, INTEGRATION.md "Interleaved generation").
//
// 1. dllm_interleave_park: the per-row stop of a decode session whose rows reach eos or <dream_start> at different steps.  One small launch
//    inside the captured token step, after the token choice: a row that has just emitted eos or the trigger id is parked, and only running
//    rows advance their position, valid cache length and cache slot.  A parked row keeps re-running its last step on one dead cache slot
//    until the host resumes it; the host reads `parked` between chunks of graph replays, never per token.
//
// 2. dllm_image_to_clip: a decoded image -> CLIP pixel values in one launch: clamp, antialiased bicubic resize of the shorter side to
//    `size` (the separable filter of torch's `interpolate(mode="bicubic", antialias=True, align_corners=False)`: support 2 * max(scale, 1)
//    source pixels around the centre scale * (i + 0.5), cubic convolution with a = -0.5, weights normalised to sum 1), centre crop,
//    (v - mean) / std.  The 8-bit round trip of the PIL processor is deliberately absent.
//    Form: one 256-thread block per 16 x 16 tile of output pixels of one (image, channel) plane.  The filter taps of the tile's 16 columns
//    and 16 rows are computed once per block into LDS; the horizontal pass then filters every source row the tile touches to the tile's 16
//    columns (one (row, column) pair per thread, each thread reading its run of contiguous source pixels with 16-byte loads between the
//    aligned bounds of the run), and the vertical pass reads those sums from LDS.  The order of the sums -- the taps of a row from left to
//    right, then the rows from top to bottom -- is the order of torch's device kernel.
#include "common.h"

namespace {

constexpr int PARK_THREADS = 64;

__global__ __launch_bounds__(PARK_THREADS) void interleave_park_kernel(const int64_t* __restrict__ tok, int B, int64_t eos, int64_t trigger,
                                                                       int advance, const int64_t* __restrict__ step, int* parked,
                                                                       int64_t* park_step, int64_t* pos, int* kv_len, int64_t* slot) {
    const int b = threadIdx.x;
    if (b >= B) return;
    int p = parked[b];
    if (p == 0) {
        const int64_t t = tok[b];
        if (eos >= 0 && t == eos) p = 1;
        else if (trigger >= 0 && t == trigger) p = 2;
        if (p != 0) {
            parked[b] = p;
            park_step[b] = *step;
        }
    }
    if (p == 0 && advance) {
        pos[b] += 1;
        kv_len[b] += 1;
        slot[b] += 1;
    }
}

constexpr int CLIP_TILE = 16;        // output pixels per block: CLIP_TILE x CLIP_TILE
constexpr int CLIP_THREADS = CLIP_TILE * CLIP_TILE;
constexpr int CLIP_MAX_TAPS = 48;    // taps per output pixel and axis: 2 * ceil(2 * scale) + 1
constexpr int CLIP_MAX_ROWS = 192;   // source rows under one tile
constexpr int CLIP_HLD = CLIP_TILE + 1;
constexpr int CLIP_WLD = CLIP_MAX_TAPS + 1;  // odd row pitch: the 16 columns of a wave read their taps from 16 banks

// cubic convolution kernel with a = -0.5 (torch's antialias bicubic filter; Keys 1981)
__device__ __forceinline__ float cubic_aa(float x) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
    return 0.0f;
}

// taps of resized pixel i along one axis: source pixels [mn, mn + n), weights w[0..n) summing to 1
__device__ __forceinline__ void clip_taps(int i, int in_size, float scale, float support, float* w, int& mn, int& n) {
    const float center = scale * ((float)i + 0.5f);
    const float invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
    mn = max((int)(center - support + 0.5f), 0);
    n = min(min((int)(center + support + 0.5f), in_size) - mn, CLIP_MAX_TAPS);
    float total = 0.f;
    for (int j = 0; j < n; ++j) {
        const float v = cubic_aa(((float)(j + mn) - center + 0.5f) * invscale);
        w[j] = v;
        total += v;
    }
    if (total != 0.f)
        for (int j = 0; j < n; ++j) w[j] /= total;
}

template <typename T>
struct ClipVec;
template <>
struct ClipVec<float> {
    static constexpr int N = 4;
    typedef f32x4 V;
    static __device__ __forceinline__ float get(const V& v, int i) { return v[i]; }
};
template <>
struct ClipVec<bf16> {
    static constexpr int N = 8;
    typedef bf16x8 V;
    static __device__ __forceinline__ float get(const V& v, int i) { return bf2f(v[i]); }
};

__device__ __forceinline__ float clip_unit(float x, int signed_range) {
    if (signed_range) x = x * 0.5f + 0.5f;
    return fminf(fmaxf(x, 0.0f), 1.0f);
}

template <typename T, typename O>
__global__ __launch_bounds__(CLIP_THREADS) void image_to_clip_kernel(const T* __restrict__ img, O* __restrict__ out, int H, int W, int RH, int RW,
                                                                     int top, int left, int size, int signed_range, int vec_ok, float m0,
                                                                     float m1, float m2, float s0, float s1, float s2) {
    __shared__ float wx[CLIP_TILE][CLIP_WLD], wy[CLIP_TILE][CLIP_WLD];
    __shared__ int xmin[CLIP_TILE], xn[CLIP_TILE], ymin[CLIP_TILE], yn[CLIP_TILE];
    __shared__ float hbuf[CLIP_MAX_ROWS * CLIP_HLD];
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, c = plane % 3;
    const int ox0 = blockIdx.x * CLIP_TILE, oy0 = blockIdx.y * CLIP_TILE;
    const float scale_w = (float)W / (float)RW, scale_h = (float)H / (float)RH;
    // ---- taps of the tile's columns (threads 0..15) and rows (threads 64..79: another wave)
    if (tid < CLIP_TILE) {
        int mn = 0, n = 0;
        if (ox0 + tid < size) clip_taps(ox0 + tid + left, W, scale_w, scale_w >= 1.0f ? 2.0f * scale_w : 2.0f, wx[tid], mn, n);
        xmin[tid] = mn;
        xn[tid] = max(n, 0);
    } else if (tid >= 64 && tid < 64 + CLIP_TILE) {
        const int t = tid - 64;
        int mn = 0, n = 0;
        if (oy0 + t < size) clip_taps(oy0 + t + top, H, scale_h, scale_h >= 1.0f ? 2.0f * scale_h : 2.0f, wy[t], mn, n);
        ymin[t] = mn;
        yn[t] = max(n, 0);
    }
    __syncthreads();
    const int rows_valid = min(CLIP_TILE, size - oy0);
    const int y0 = ymin[0];
    int y1 = y0;
    for (int t = 0; t < rows_valid; ++t) y1 = max(y1, ymin[t] + yn[t]);
    const int nrows = min(y1 - y0, CLIP_MAX_ROWS);  // (the launcher has checked that the tile fits; the clamp only keeps LDS in bounds)
    const T* src = img + (int64_t)plane * H * W;
    // ---- horizontal pass: hbuf[r][ox] = sum_j wx[ox][j] * src[y0 + r][xmin[ox] + j]
    constexpr int VN = ClipVec<T>::N;
    for (int idx = tid; idx < nrows * CLIP_TILE; idx += CLIP_THREADS) {
        const int r = idx / CLIP_TILE, ox = idx % CLIP_TILE;
        const int n = xn[ox];
        const int64_t e0 = (int64_t)(y0 + r) * W + xmin[ox];  // element index inside the plane; the plane base is VN-aligned when vec_ok
        const T* p = src + e0;
        const float* w = wx[ox];
        float acc = 0.f;
        int j = 0;
        if (vec_ok) {
            const int lead = min((int)((VN - (e0 & (VN - 1))) & (VN - 1)), n);
            for (; j < lead; ++j) acc += w[j] * clip_unit((float)p[j], signed_range);
            for (; j + VN <= n; j += VN) {
                const typename ClipVec<T>::V v = *reinterpret_cast<const typename ClipVec<T>::V*>(p + j);
#pragma unroll
                for (int e = 0; e < VN; ++e) acc += w[j + e] * clip_unit(ClipVec<T>::get(v, e), signed_range);
            }
        }
        for (; j < n; ++j) acc += w[j] * clip_unit((float)p[j], signed_range);
        hbuf[r * CLIP_HLD + ox] = acc;
    }
    __syncthreads();
    // ---- vertical pass, normalise, store
    const int tx = tid % CLIP_TILE, ty = tid / CLIP_TILE;
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= size || oy >= size) return;
    const int r0 = ymin[ty] - y0, n = min(yn[ty], nrows - r0);
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc += wy[ty][j] * hbuf[(r0 + j) * CLIP_HLD + tx];
    const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    out[((int64_t)plane * size + oy) * size + ox] = (O)((acc - mean) / sd);
}

template <typename T, typename O>
static void launch_clip(dim3 g, hipStream_t s, const void* img, void* out, int H, int W, int RH, int RW, int top, int left, int size, int sr,
                        int vec_ok, const float* m, const float* sd) {
    hipLaunchKernelGGL((image_to_clip_kernel<T, O>), g, dim3(CLIP_THREADS), 0, s, static_cast<const T*>(img), static_cast<O*>(out), H, W, RH, RW,
                       top, left, size, sr, vec_ok, m[0], m[1], m[2], sd[0], sd[1], sd[2]);
}

}  // namespace

extern "C" int dllm_interleave_park(const int64_t* tok, int B, int64_t eos, int64_t trigger, int advance, const int64_t* step, int* parked,
                                    int64_t* park_step, int64_t* pos, int* kv_len, int64_t* slot, void* stream) {
    if (B < 0 || B > PARK_THREADS || tok == nullptr || step == nullptr || parked == nullptr || park_step == nullptr) return DLLM_ERR_SHAPE;
    if (advance && (pos == nullptr || kv_len == nullptr || slot == nullptr)) return DLLM_ERR_SHAPE;
    if (B == 0) return DLLM_OK;
    hipLaunchKernelGGL(interleave_park_kernel, dim3(1), dim3(PARK_THREADS), 0, (hipStream_t)stream, tok, B, eos, trigger, advance, step, parked,
                       park_step, pos, kv_len, slot);
    return dllm_check_launch();
}

extern "C" int dllm_image_to_clip(const void* image, void* out, int B, int H, int W, int size, int in_dtype, int out_dtype, int signed_range,
                                  float mean0, float mean1, float mean2, float std0, float std1, float std2, void* stream) {
    if (B < 0 || H <= 0 || W <= 0 || size <= 0 || image == nullptr || out == nullptr) return DLLM_ERR_SHAPE;
    if (!(std0 != 0.f && std1 != 0.f && std2 != 0.f)) return DLLM_ERR_SHAPE;
    if ((in_dtype != DLLM_BF16 && in_dtype != DLLM_F32) || (out_dtype != DLLM_BF16 && out_dtype != DLLM_F32)) return DLLM_ERR_DTYPE;
    if ((int64_t)B * 3 > 65535) return DLLM_ERR_SHAPE;
    // the shorter side goes to `size`, the longer one keeps the aspect ratio (truncated), the crop is centred
    const int RH = H <= W ? size : (int)((int64_t)size * H / W), RW = H <= W ? (int)((int64_t)size * W / H) : size;
    const int top = (RH - size) / 2, left = (RW - size) / 2;
    // what one tile needs of the source must fit the block's LDS: taps per pixel, and the source rows under 16 output rows
    const float scale_h = (float)H / (float)RH, scale_w = (float)W / (float)RW;
    const float sup_h = scale_h >= 1.f ? 2.f * scale_h : 2.f, sup_w = scale_w >= 1.f ? 2.f * scale_w : 2.f;
    const int taps_h = 2 * (int)ceilf(sup_h) + 1, taps_w = 2 * (int)ceilf(sup_w) + 1;
    if (taps_h > CLIP_MAX_TAPS || taps_w > CLIP_MAX_TAPS) return DLLM_ERR_SHAPE;
    if ((int)ceilf((CLIP_TILE - 1) * scale_h) + taps_h + 2 > CLIP_MAX_ROWS) return DLLM_ERR_SHAPE;
    if (B == 0) return DLLM_OK;
    const int vn = in_dtype == DLLM_F32 ? 4 : 8;
    // 16-byte loads need every plane to start on a 16-byte boundary (runs inside a plane are aligned per thread)
    const int vec_ok = ((uintptr_t)image % 16 == 0) && (((int64_t)H * W) % vn == 0);
    const dim3 g((unsigned)((size + CLIP_TILE - 1) / CLIP_TILE), (unsigned)((size + CLIP_TILE - 1) / CLIP_TILE), (unsigned)(B * 3));
    hipStream_t s = (hipStream_t)stream;
    const float m[3] = {mean0, mean1, mean2}, sd[3] = {std0, std1, std2};
    if (in_dtype == DLLM_F32 && out_dtype == DLLM_F32) launch_clip<float, float>(g, s, image, out, H, W, RH, RW, top, left, size, signed_range, vec_ok, m, sd);
    else if (in_dtype == DLLM_F32) launch_clip<float, bf16>(g, s, image, out, H, W, RH, RW, top, left, size, signed_range, vec_ok, m, sd);
    else if (out_dtype == DLLM_F32) launch_clip<bf16, float>(g, s, image, out, H, W, RH, RW, top, left, size, signed_range, vec_ok, m, sd);
    else launch_clip<bf16, bf16>(g, s, image, out, H, W, RH, RW, top, left, size, signed_range, vec_ok, m, sd);
    return dllm_check_launch();
}
