// Scheduler step of the graphed denoising loop for any (DDPM / DDIM) scheduler, with or without classifier-free guidance and with
// the guidance rescale of modeling_plugins.py:658-669, in ONE launch per step.  Replaces the plain loop's chunk + CFG combine
// (:824-828), `_rescale_noise_cfg` (:829-830), `scheduler.step` (:833) and the next iteration's torch.cat([latents] * G) + cast
// (:811-812).  The scheduler's step is passed as host coefficients (schedulers.py `step_coeffs`):
//   e      = e_u + s (e_c - e_u)                        (G = 2; G = 1: e = pred)
//   e      = phi e std(e_c) / std(e) + (1 - phi) e      (phi > 0; unbiased std per image over its 4 P values)
//   x0     = (x - s1a e) / sa,  eps = e                 [epsilon]     x0 = sa x - s1a e,  eps = sa e + s1a x   [v-prediction]
//   x_prev = k_x0 x0 + k_eps eps + k_x x + sigma z      (z: noise, read only when sigma != 0)
// pred: bf16 [G B][P][4] NHWC (uncond half first), lat: fp32 [B][P][4] in place, noise: fp32 [B][P][4] or null,
// next_in: bf16 [G B][P][8] (channels 4..7 zero: the conv_in operand of the next step) or null.
// Form: without rescale one thread per latent pixel, grid-stride.  With rescale one 512-thread block per image: two passes over
// the image for the means and the centred sums of squares (fixed-order wave + block reductions, no atomics: two launches give the
// same bits), then the update pass.  ~40-60 B per pixel: HBM / launch-latency bound.
//
// `dllm_cfg_dpm_step` is the same step for a second-order multistep scheduler (schedulers.py `multistep_coeffs`: DPM-Solver++),
// whose update also needs the data prediction of the step before.  That history lives in an fp32 buffer hist [B][P][4] which
// every launch overwrites with its own m0 and the next launch reads as m1:
//   m0     = (x - s1a e) / sa  [epsilon]     m0 = sa x - s1a e  [v-prediction]        (e guided and rescaled as above)
//   x_next = k_x x + k_m0 m0 + k_m1 m1 + sigma z      (m1: hist, read only when k_m1 != 0 -- on the first step it is uninitialised;
//                                                       z: noise, read only when sigma != 0)
// Same two forms; +16 B read and +16 B written per pixel.
#include "common.h"

#include <type_traits>

namespace {

constexpr int SCHED_THREADS = 256;
constexpr int RESCALE_THREADS = 512;
constexpr int RESCALE_WAVES = RESCALE_THREADS / 64;

struct SchedArgs {
    const bf16* pred;
    float* lat;
    const float* noise;
    bf16* next_in;
    int64_t B, P;
    int G, vpred;
    float gs, phi, sa, s1a, k_x0, k_eps, k_x, sigma;
};

struct DpmArgs {
    const bf16* pred;
    float* lat;
    float* hist;
    const float* noise;
    bf16* next_in;
    int64_t B, P;
    int G, vpred;
    float gs, phi, sa, s1a, k_x, k_m0, k_m1, sigma;
};

// guided prediction of pixel i (flat b * P + p) and the conditional half's values (G = 1: both are pred)
template <typename Args>
__device__ __forceinline__ void guided(const Args& a, int64_t i, f32x4& e, f32x4& ec) {
    if (a.G == 2) {
        const bf16x4 u = ld_bf16x4(a.pred + i * 4), c = ld_bf16x4(a.pred + (a.B * a.P + i) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ec[k] = (float)c[k];
            e[k] = (float)u[k] + a.gs * (ec[k] - (float)u[k]);
        }
    } else {
        const bf16x4 c = ld_bf16x4(a.pred + i * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = ec[k] = (float)c[k];
    }
}

// scheduler update of pixel i from its guided (and rescaled) prediction
__device__ __forceinline__ void update(const SchedArgs& a, int64_t i, f32x4 e) {
    f32x4 x = *reinterpret_cast<f32x4*>(a.lat + i * 4);
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (a.sigma != 0.f) z = *reinterpret_cast<const f32x4*>(a.noise + i * 4);
    bf16x8 o = zero_bf16x8();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float x0, eps;
        if (a.vpred) {
            x0 = a.sa * x[c] - a.s1a * e[c];
            eps = a.sa * e[c] + a.s1a * x[c];
        } else {
            x0 = (x[c] - a.s1a * e[c]) / a.sa;
            eps = e[c];
        }
        x[c] = a.k_x0 * x0 + a.k_eps * eps + a.k_x * x[c] + a.sigma * z[c];
        o[c] = (bf16)x[c];
    }
    *reinterpret_cast<f32x4*>(a.lat + i * 4) = x;
    if (a.next_in != nullptr)
        for (int g = 0; g < a.G; ++g) st_bf16x8(a.next_in + (g * a.B * a.P + i) * 8, o);
}

// multistep update of pixel i from its guided (and rescaled) prediction; hist: m1 in (only when it has a weight), m0 out
__device__ __forceinline__ void update(const DpmArgs& a, int64_t i, f32x4 e) {
    f32x4 x = *reinterpret_cast<f32x4*>(a.lat + i * 4);
    f32x4 m1 = {0.f, 0.f, 0.f, 0.f}, z = {0.f, 0.f, 0.f, 0.f};
    if (a.k_m1 != 0.f) m1 = *reinterpret_cast<const f32x4*>(a.hist + i * 4);
    if (a.sigma != 0.f) z = *reinterpret_cast<const f32x4*>(a.noise + i * 4);
    f32x4 m0;
    bf16x8 o = zero_bf16x8();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        m0[c] = a.vpred ? a.sa * x[c] - a.s1a * e[c] : (x[c] - a.s1a * e[c]) / a.sa;
        x[c] = a.k_x * x[c] + a.k_m0 * m0[c] + a.k_m1 * m1[c] + a.sigma * z[c];
        o[c] = (bf16)x[c];
    }
    *reinterpret_cast<f32x4*>(a.lat + i * 4) = x;
    *reinterpret_cast<f32x4*>(a.hist + i * 4) = m0;
    if (a.next_in != nullptr)
        for (int g = 0; g < a.G; ++g) st_bf16x8(a.next_in + (g * a.B * a.P + i) * 8, o);
}

// one thread per latent pixel, grid-stride
template <typename Args>
__global__ __launch_bounds__(SCHED_THREADS) void cfg_step_kernel(Args a) {
    const int64_t n = a.B * a.P;
    for (int64_t i = (int64_t)blockIdx.x * SCHED_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SCHED_THREADS) {
        f32x4 e, ec;
        guided(a, i, e, ec);
        update(a, i, e);
    }
}

// block sum of two values in a fixed order (every thread receives the result)
__device__ __forceinline__ f32x2 block_sum2(f32x2 v, f32x2* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v[0] += __shfl_xor(v[0], o, 64);
        v[1] += __shfl_xor(v[1], o, 64);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    f32x2 s = red[0];
#pragma unroll
    for (int k = 1; k < RESCALE_WAVES; ++k) s += red[k];
    __syncthreads();
    return s;
}

// one block per image, three passes (verified: each instantiation compiles to the instruction stream and registers of a hand-written copy)
template <typename Args>
__global__ __launch_bounds__(RESCALE_THREADS) void cfg_step_rescale_kernel(Args a) {
    __shared__ f32x2 red[RESCALE_WAVES];
    const int64_t base = (int64_t)blockIdx.x * a.P;
    const float cnt = (float)(a.P * 4);
    // pass 1: means of the conditional prediction and of the guided one
    f32x2 s = {0.f, 0.f};
    for (int64_t p = threadIdx.x; p < a.P; p += RESCALE_THREADS) {
        f32x4 e, ec;
        guided(a, base + p, e, ec);
        s[0] += (ec[0] + ec[1]) + (ec[2] + ec[3]);
        s[1] += (e[0] + e[1]) + (e[2] + e[3]);
    }
    const f32x2 mean = block_sum2(s, red) / cnt;
    // pass 2: centred sums of squares
    f32x2 q = {0.f, 0.f};
    for (int64_t p = threadIdx.x; p < a.P; p += RESCALE_THREADS) {
        f32x4 e, ec;
        guided(a, base + p, e, ec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dc = ec[k] - mean[0], de = e[k] - mean[1];
            q[0] += dc * dc;
            q[1] += de * de;
        }
    }
    const f32x2 ss = block_sum2(q, red);
    const float ratio = sqrtf(ss[0] / (cnt - 1.f)) / sqrtf(ss[1] / (cnt - 1.f));  // std(e_c) / std(e)
    // pass 3: rescale + update
    for (int64_t p = threadIdx.x; p < a.P; p += RESCALE_THREADS) {
        f32x4 e, ec;
        guided(a, base + p, e, ec);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = a.phi * (e[k] * ratio) + (1.f - a.phi) * e[k];
        update(a, base + p, e);
    }
}

// What the two entry points share: the argument checks, the common fields, and the launch -- with rescale one block per image, else
// grid-stride capped at 8192 blocks.  `a` arrives with the scheduler's own fields set (for DpmArgs that includes hist).
template <typename Args>
int cfg_step(Args& a, const void* pred, float* latents, const float* noise, void* next_in, int64_t B, int64_t P, int G, float guidance,
             float rescale, int v_prediction, float sqrt_at, float sqrt_1mat, float sigma, void* stream) {
    const float* hist = latents;  // no history: nothing more to check
    if constexpr (std::is_same_v<Args, DpmArgs>) hist = a.hist;
    if (B < 0 || P < 0 || B > 0x7FFFFFFFLL || (G != 1 && G != 2) || !(rescale >= 0.f) || (rescale > 0.f && P * 4 < 2))
        return DLLM_ERR_SHAPE;
    if (B == 0 || P == 0) return DLLM_OK;
    if (pred == nullptr || latents == nullptr || hist == nullptr || (sigma != 0.f && noise == nullptr)) return DLLM_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(pred) & 7 || reinterpret_cast<uintptr_t>(latents) & 15 || reinterpret_cast<uintptr_t>(hist) & 15 ||
        reinterpret_cast<uintptr_t>(noise) & 15 || reinterpret_cast<uintptr_t>(next_in) & 15)
        return DLLM_ERR_ALIGN;
    a.pred = (const bf16*)pred;
    a.lat = latents;
    a.noise = noise;
    a.next_in = (bf16*)next_in;
    a.B = B;
    a.P = P;
    a.G = G;
    a.vpred = v_prediction ? 1 : 0;
    a.gs = guidance;
    a.phi = rescale;
    a.sa = sqrt_at;
    a.s1a = sqrt_1mat;
    a.sigma = sigma;
    hipStream_t s = (hipStream_t)stream;
    if (rescale > 0.f) {
        hipLaunchKernelGGL(cfg_step_rescale_kernel<Args>, dim3((unsigned)B), dim3(RESCALE_THREADS), 0, s, a);
    } else {
        int64_t g = cdiv64(B * P, SCHED_THREADS);
        if (g > 8192) g = 8192;  // grid-stride the rest
        hipLaunchKernelGGL(cfg_step_kernel<Args>, dim3((unsigned)g), dim3(SCHED_THREADS), 0, s, a);
    }
    return dllm_check_launch();
}

}  // namespace

extern "C" int dllm_cfg_sched_step(const void* pred, float* latents, const float* noise, void* next_in, int64_t B, int64_t P, int G,
                                   float guidance, float rescale, int v_prediction, float sqrt_at, float sqrt_1mat, float k_x0,
                                   float k_eps, float k_x, float sigma, void* stream) {
    SchedArgs a;
    a.k_x0 = k_x0;
    a.k_eps = k_eps;
    a.k_x = k_x;
    return cfg_step(a, pred, latents, noise, next_in, B, P, G, guidance, rescale, v_prediction, sqrt_at, sqrt_1mat, sigma, stream);
}

extern "C" int dllm_cfg_dpm_step(const void* pred, float* latents, float* hist, const float* noise, void* next_in, int64_t B, int64_t P,
                                 int G, float guidance, float rescale, int v_prediction, float sqrt_at, float sqrt_1mat, float k_x,
                                 float k_m0, float k_m1, float sigma, void* stream) {
    DpmArgs a;
    a.hist = hist;
    a.k_x = k_x;
    a.k_m0 = k_m0;
    a.k_m1 = k_m1;
    return cfg_step(a, pred, latents, noise, next_in, B, P, G, guidance, rescale, v_prediction, sqrt_at, sqrt_1mat, sigma, stream);
}
