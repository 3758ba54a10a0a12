// Sampled token choice of the decode loop: temperature, top-k, top-p and the draw in ONE launch per token step, with the step's
// bookkeeping (teacher forcing, HF's finished-row rule, the token writes, the step counter) fused in.
//
// Reference call sites: omni/eval/language_eval/modeling_dreamllm.py:36-43,86-91 (`sample_top_p`, temperature 0.8 / top-p 0.95),
// omni/eval/vqa/vqa_inference.py:111-137 (`model.generate(do_sample=True, temperature=0.2)`: transformers 4.35.2 [ext]
// TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial).
//
// Semantics per row b (the tests restate them in fp64):
//   1. s_i = logits[b][i] * (1 / T) in fp32, for i < V (V = vocabulary limit; ids >= V are never emitted).
//   2. top-k (0 < k < V): keep i iff s_i >= s_(k), the k-th largest value; ties at the boundary are all kept (TopKLogitsWarper).
//   3. top-p (p < 1): over the kept set, q = softmax(s); keep i iff sum_{kept j: q_j > q_i} q_j <= p (the language loop's
//      `probs_sum - probs_sort > p` rule, ties treated alike).  HF 4.35's TopPLogitsWarper keeps i iff that sum is < p; the two
//      differ only at exact equality.  The maximum is always kept; p <= 0 keeps the arg-max ties.
//   4. draw: one uniform u in [0, 1) per row; the token is the smallest kept i (vocabulary order) with
//      sum_{kept j <= i} q_j > u * sum_kept q_j.  Masked (-inf, zero-mass) ids are never drawn.
//   5. u: caller-supplied `uniforms[b]`, or Philox4x32-10 (Random123) with key = the 64-bit *seed, counter =
//      (b, step_lo, step_hi, 0) and u = (x0 >> 8) * 2^-24.  Seed and step are read from device memory, so a captured graph
//      draws fresh numbers on every replay.
//   6. a row whose maximum is not finite or that holds a NaN emits id 0 and sets status[b] = 1 (sticky; never cleared here).
//   7. bookkeeping, in this order: teacher forcing (force_mask[step][b] -> force_tok[step][b]); then, with eos >= 0, a row with
//      finished[b] set emits `pad`, and a row that emits eos by its own choice (not forced) sets finished[b];
//      out_tokens[step][b] = tok_out[b] = the token; with step_inc, the last block to finish adds 1 to *step.
//
// Form: one 1024-thread block per row, V <= 32768.  Thread t owns the CONTIGUOUS ids [t * EPT, (t + 1) * EPT) (so that thread order is
// vocabulary order for the draw's scan), held in registers as the order-preserving uint32 key of s plus q = exp(s - max)
// (32 + 32 VGPRs at V > 8192: the kernel sits at 128 VGPRs without scratch; ids that top-k drops get key 0 = out of play).
// Both thresholds are searched two bits at a time on the key (16 rounds each, three candidates per round): top-k with exact
// integer counts, top-p with fp32 masses.  Every float sum is per-thread sequential, a butterfly within the wave (every lane
// ends with the same bits) and the 16 wave totals added in a fixed order -- no float atomics, bit-identical on every launch.
// The computed masses are monotone in the candidate threshold (rounding is monotone), so the searches are well defined.
#include "common.h"

namespace {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;

__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// Philox4x32-10 (Salmon et al., SC'11; the Random123 reference constants): 10 rounds, the key bumped between rounds.
__device__ __forceinline__ uint32_t philox_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// N block sums at once (deterministic: wave butterfly, then the wave totals in wave order).  scratch: N * SAMPLE_WAVES floats.
template <int N>
__device__ __forceinline__ void block_sums(float (&v)[N], float* scratch) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = wave_sum(v[n]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) scratch[n * SAMPLE_WAVES + w] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) {
        float r = 0.f;
#pragma unroll
        for (int i = 0; i < SAMPLE_WAVES; ++i) r += scratch[n * SAMPLE_WAVES + i];
        v[n] = r;
    }
}

template <int EPT>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_logits_kernel(
    const float* __restrict__ logits, int64_t ld, int B, int V, float temperature, int top_k, float top_p,
    const int64_t* __restrict__ seed, int64_t* step, int* arrive, int step_inc, const float* __restrict__ uniforms,
    const int64_t* __restrict__ force_tok, const bool* __restrict__ force_mask, int64_t n_steps, int64_t eos, int64_t pad,
    bool* finished, int64_t* out_tokens, int64_t* tok_out, float* u_out, int* kept_out, int* status) {
    __shared__ float scratch[3 * SAMPLE_WAVES];
    __shared__ float wave_tot[SAMPLE_WAVES];
    __shared__ int s_flag, s_cand, s_last, s_kept;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (int64_t)b * ld;
    const float inv_t = 1.0f / temperature;
    const int i0 = tid * EPT;
    if (tid == 0) {
        s_flag = 0;
        s_cand = 0x7FFFFFFF;
        s_last = -1;
        s_kept = 0;
    }
    // ---- load, scale, max (key 0 = padding: below every non-NaN value)
    uint32_t key[EPT];
    float q[EPT];
    float mx = -INFINITY;
    bool nan = false;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int i = i0 + j;
        key[j] = 0u;
        if (i < V) {
            const float x = row[i];
            nan |= x != x;
            const float s = x * inv_t;
            key[j] = f2key(s);
            mx = fmaxf(mx, s);
        }
    }
    mx = block_max<SAMPLE_WAVES>(mx, scratch);
    if (nan) atomicOr(&s_flag, 1);
    __syncthreads();
    const bool bad = s_flag != 0 || !(fabsf(mx) <= 3.402823466e38f);
    if (!bad) {
        auto qv = [&](int j) -> float { return key[j] ? q[j] : 0.f; };
#pragma unroll
        for (int j = 0; j < EPT; ++j) q[j] = key[j] ? __expf(key2f(key[j]) - mx) : 0.f;
        // ---- top-k: the largest t with #(key >= t) >= k is the k-th largest key
        uint32_t tk = 1u;
        if (top_k > 0 && top_k < V) {
            uint32_t t = 0u;
            for (int sh = 30; sh >= 0; sh -= 2) {
                float c[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < EPT; ++j) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) c[d] += key[j] >= (t | ((uint32_t)(d + 1) << sh)) ? 1.f : 0.f;
                }
                block_sums<3>(c, scratch);
                uint32_t d = 0;
#pragma unroll
                for (int e = 0; e < 3; ++e) d = c[e] >= (float)top_k ? (uint32_t)(e + 1) : d;
                t |= d << sh;
            }
            tk = t;
#pragma unroll
            for (int j = 0; j < EPT; ++j) key[j] = key[j] >= tk ? key[j] : 0u;  // the rest is out of play from here on
        }
        // ---- top-p: the largest t with mass(kept, key > t) > p * mass(kept); kept = key > t
        uint32_t tp = 0u;
        if (top_p < 1.0f) {
            float zk[1] = {0.f};
#pragma unroll
            for (int j = 0; j < EPT; ++j) zk[0] += qv(j);
            block_sums<1>(zk, scratch);
            const float lim = fmaxf(top_p, 0.f) * zk[0];
            uint32_t t = 0u;
            for (int sh = 30; sh >= 0; sh -= 2) {
                float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < EPT; ++j) {
                    const float qj = qv(j);
#pragma unroll
                    for (int d = 0; d < 3; ++d) g[d] += key[j] > (t | ((uint32_t)(d + 1) << sh)) ? qj : 0.f;
                }
                block_sums<3>(g, scratch);
                uint32_t d = 0;
#pragma unroll
                for (int e = 0; e < 3; ++e) d = g[e] > lim ? (uint32_t)(e + 1) : d;
                t |= d << sh;
            }
            tp = t + 1u;
        }
        const uint32_t thr = tk > tp ? tk : tp;  // kept: key >= thr
        // ---- draw: exclusive scan of the kept mass in vocabulary order
        float c = 0.f;
        int nk = 0;
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const bool kp = key[j] >= thr;
            c += kp ? qv(j) : 0.f;
            nk += kp ? 1 : 0;
        }
        const int lane = tid & 63, w = tid >> 6;
        float inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        float excl = __shfl_up(inc, 1, 64);
        if (lane == 0) excl = 0.f;
        if (lane == 63) wave_tot[w] = inc;
        if (nk) atomicAdd(&s_kept, nk);
        __syncthreads();
        float off = 0.f, total = 0.f;
#pragma unroll
        for (int i = 0; i < SAMPLE_WAVES; ++i) {
            off += i < w ? wave_tot[i] : 0.f;
            total += wave_tot[i];
        }
        float u;
        if (uniforms != nullptr) {
            u = uniforms[b];
        } else {
            const uint64_t st = (uint64_t)*step, sd = (uint64_t)*seed;
            const uint32_t x0 = philox_x0((uint32_t)b, (uint32_t)st, (uint32_t)(st >> 32), 0u, (uint32_t)sd, (uint32_t)(sd >> 32));
            u = (float)(x0 >> 8) * 5.9604644775390625e-8f;
        }
        const float target = u * total;
        float run = off + excl;
        int cand = 0x7FFFFFFF, last = -1;
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const float qj = qv(j);
            if (key[j] >= thr && qj > 0.f) {
                run += qj;
                last = i0 + j;
                if (run > target && cand == 0x7FFFFFFF) cand = i0 + j;
            }
        }
        if (cand != 0x7FFFFFFF) atomicMin(&s_cand, cand);
        if (last >= 0) atomicMax(&s_last, last);
        if (tid == 0 && u_out != nullptr) u_out[b] = u;
        __syncthreads();
    } else if (tid == 0 && u_out != nullptr) {
        u_out[b] = uniforms != nullptr ? uniforms[b] : 0.f;
    }
    if (tid != 0) return;
    // ---- bookkeeping (one thread)
    int64_t tok = 0;
    if (bad) {
        status[b] = 1;
    } else {
        tok = s_cand != 0x7FFFFFFF ? s_cand : (s_last >= 0 ? s_last : 0);  // the fallback: rounding of u * total at u -> 1
    }
    if (kept_out != nullptr) kept_out[b] = bad ? 0 : s_kept;
    const int64_t st = *step;
    const bool in_range = st >= 0 && st < n_steps;
    bool forced = false;
    if (force_mask != nullptr && in_range && force_mask[st * B + b]) {
        tok = force_tok[st * B + b];
        forced = true;
    }
    if (eos >= 0 && finished != nullptr) {
        if (finished[b]) tok = pad;
        else if (!forced && tok == eos) finished[b] = true;
    }
    if (out_tokens != nullptr && in_range) out_tokens[st * B + b] = tok;
    if (tok_out != nullptr) tok_out[b] = tok;
    if (step_inc) {
        // every block has read *step above (its value is already consumed); the last block to arrive advances it
        __threadfence();
        if (atomicAdd(arrive, 1) == B - 1) {
            *arrive = 0;
            *step = st + 1;
        }
    }
}

template <int EPT>
static void launch_sample(dim3 g, hipStream_t s, const float* logits, int64_t ld, int B, int V, float T, int k, float p, const int64_t* seed,
                          int64_t* step, int* arrive, int inc, const float* uniforms, const int64_t* ft, const bool* fm, int64_t n_steps,
                          int64_t eos, int64_t pad, bool* fin, int64_t* out, int64_t* tok, float* u_out, int* kept, int* status) {
    hipLaunchKernelGGL(sample_logits_kernel<EPT>, g, dim3(SAMPLE_THREADS), 0, s, logits, ld, B, V, T, k, p, seed, step, arrive, inc, uniforms,
                       ft, fm, n_steps, eos, pad, fin, out, tok, u_out, kept, status);
}

}  // namespace

extern "C" int dllm_sample_logits(const float* logits, int64_t ld, int B, int V, float temperature, int top_k, float top_p,
                                  const int64_t* seed, int64_t* step, int* arrive, int step_inc, const float* uniforms,
                                  const int64_t* force_tok, const void* force_mask, int64_t n_steps, int64_t eos, int64_t pad,
                                  void* finished, int64_t* out_tokens, int64_t* tok_out, float* u_out, int* kept_out, int* status,
                                  void* stream) {
    if (B < 0 || V <= 0 || V > 32 * SAMPLE_THREADS || ld < V || !(temperature > 0.f) || step == nullptr || status == nullptr)
        return DLLM_ERR_SHAPE;
    if ((uniforms == nullptr && seed == nullptr) || (step_inc && arrive == nullptr) || (force_mask != nullptr && force_tok == nullptr) ||
        (eos >= 0 && finished == nullptr) || n_steps < 0)
        return DLLM_ERR_SHAPE;
    if (B == 0) return DLLM_OK;
    const dim3 g((unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    auto* fm = static_cast<const bool*>(force_mask);
    auto* fin = static_cast<bool*>(finished);
    if (V <= 8 * SAMPLE_THREADS)
        launch_sample<8>(g, s, logits, ld, B, V, temperature, top_k, top_p, seed, step, arrive, step_inc, uniforms, force_tok, fm, n_steps, eos,
                         pad, fin, out_tokens, tok_out, u_out, kept_out, status);
    else
        launch_sample<32>(g, s, logits, ld, B, V, temperature, top_k, top_p, seed, step, arrive, step_inc, uniforms, force_tok, fm, n_steps, eos,
                          pad, fin, out_tokens, tok_out, u_out, kept_out, status);
    return dllm_check_launch();
}
