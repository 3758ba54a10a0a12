// Scoring of given text: per row of fp32 logits the log-probability of a target id, the row's log-sum-exp, its arg-max, the
// target's rank and the log-probabilities of a small candidate set, in ONE launch that reads each row once; and the per-request
// sums over row segments.  This is what `loglikelihood()` / `choice_logprobs()` run above the chunked fp32 lm_head GEMM.
//
// Reference call sites: omni/eval/language_eval/submission_scripts/submission_dev_{hellaswag,piqa,siqa,boolq,winogrande}.py and
// llama_evaluation_main/.../evaluator_utils.py:124-137 (`log_softmax(logits.cpu().float())`, `gather` at rows [-n-1:-1]);
// omni/eval/language_eval/eval_mmlu.py:43-62, evaluate_mmlu.py:62-87 (`logits[:, -1]` at the ids of "A".."D");
// language_eval/modeling_dreamllm.py:79,86 (`logits[..., :32000]`: V here is that limit).
//
// Semantics per row r with t = targets[r], over the ids i < V (the tests restate them in fp64):
//   lse     = max + log sum_i exp(x_i - max)
//   logprob = (x_t - max) - log sum_i exp(x_i - max)
//   argmax  = the lowest i with x_i = max (torch.argmax; -0.0 and +0.0 are equal, as in every float comparison)
//   greedy  = argmax == t
//   rank    = #{i : x_i > x_t} + #{i < t : x_i == x_t}                       (0 <=> greedy)
//   cand_logprob[k] = x_{cand_ids[k]} - lse                                  (K <= 16 ids shared by all rows)
// Rows that cannot be scored are reported, never faulted on:
//   t < 0  (row not scored)  logprob 0, greedy 0, rank -1; lse / argmax / candidates are still written
//   t >= V (bad device data) logprob -inf, greedy 0, rank -1, status |= 1
//   a NaN or +inf in the row, or no finite value at all: lse and candidates NaN, argmax 0, greedy 0, rank -1, logprob NaN (for a
//   target in [0, V); the two rules above keep their logprob), status |= 2
//   a candidate id outside [0, V) (the Python layer rejects it before the launch): NaN, nothing is read
//
// Form: one block per row.  The row is loaded once, as 16-byte vectors interleaved over the threads (vector q of the row belongs
// to thread q % THREADS: coalesced), and stays in registers (NV vectors = 4 NV values per thread; 1024 threads x 8 vectors cover
// V <= 32768 in 32 of the kernel's 55 VGPRs, so two blocks fit a CU and 8 loads per thread are in flight before the first use).  x_t is a direct load;
// one sweep over the registers gives the thread's maximum with its first index and the rank count, one block reduction combines
// them (64-bit key = order-preserving value bits, then ~index: an order, so the result does not depend on how it is reduced;
// integer counts; the ids after the last whole vector, V % 4 of them, are swept by thread 0 after its own), a second sweep over the same registers gives sum exp(x - max).  V > 32768 takes the same code with the
// registers replaced by a re-read of the row (NV = 0: three reads, two of them from cache; correctness, not speed).
// Float sums: per thread in register order, a butterfly within the wave (every lane ends with the same bits), then the wave
// totals in wave order -- no float atomics, bit-identical on every launch.  The status word takes an integer atomic OR.
#include "common.h"

namespace {

constexpr int SCORE_MAX_CAND = 16;

__device__ __forceinline__ uint32_t score_key(float f) {
    uint32_t b = __float_as_uint(f);
    if (b == 0x80000000u) b = 0u;  // -0.0 == +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = (uint64_t)__shfl_xor((long long)v, o, 64);
        v = y > v ? y : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the four values of vector q of a row (columns 4 q .. 4 q + 3) if all of them are ids < V, else -inf, which enters no result; the
// V % 4 ids after the last whole vector are thread 0's `score_tail`
__device__ __forceinline__ f32x4 score_load(const float* __restrict__ row, int q, int V) {
    f32x4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (q * 4 + 3 < V) v = *reinterpret_cast<const f32x4*>(row + q * 4);
    return v;
}
__device__ __forceinline__ f32x4 score_tail(const float* __restrict__ row, int V) {
    f32x4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const int c = V & ~3;
#pragma unroll
    for (int e = 0; e < 3; ++e)
        if (c + e < V) v[e] = row[c + e];
    return v;
}

template <int THREADS, int NV>
__global__ __launch_bounds__(THREADS, THREADS == 1024 ? 8 : 1) void score_rows_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                             const int64_t* __restrict__ targets, float* __restrict__ logprob,
                                                             float* __restrict__ lse_out, int64_t* __restrict__ argmax_out,
                                                             uint8_t* __restrict__ greedy_out, int* __restrict__ rank_out,
                                                             const int64_t* __restrict__ cand_ids, int n_cand,
                                                             float* __restrict__ cand_logprob, int* status) {
    constexpr int NW = THREADS / 64;
    __shared__ uint64_t s_key[NW];
    __shared__ int s_cnt[NW], s_bad[NW];
    __shared__ float s_sum[NW];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* row = logits + r * ld;
    const int64_t t = targets[r];
    const bool has_t = t >= 0 && t < V;
    const float xt = has_t ? row[t] : __uint_as_float(0x7FC00000u);  // NaN compares false with everything: nothing is counted
    const int ti = has_t ? (int)t : -1;
    const int nvec = NV > 0 ? NV : ((V + 3) / 4 + THREADS - 1) / THREADS;

    f32x4 reg[NV > 0 ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) reg[k] = score_load(row, tid + k * THREADS, V);
    }
    auto vec = [&](int k) -> f32x4 {
        if constexpr (NV > 0) return reg[k];
        else return score_load(row, tid + k * THREADS, V);
    };

    // ---- sweep 1: maximum with its first index (a thread's columns ascend with k and e), rank count, NaN / +inf
    float mx = -INFINITY;
    int mi = 0x7FFFFFFF, cnt = 0;
    bool bad = false;
    auto sweep = [&](const f32x4& v, int c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = v[e];
            bad |= !(x < INFINITY);
            if (x > mx) {
                mx = x;
                mi = c + e;
            }
            cnt += (x > xt) ? 1 : 0;
            cnt += (x == xt && c + e < ti) ? 1 : 0;
        }
    };
#pragma unroll
    for (int k = 0; k < nvec; ++k) sweep(vec(k), (tid + k * THREADS) * 4);
    const bool own_tail = tid == 0 && (V & 3) != 0;  // the row's last ids: after every other id of thread 0, so first-index order holds
    if (own_tail) sweep(score_tail(row, V), V & ~3);
    uint64_t key = ((uint64_t)score_key(mx) << 32) | (uint32_t)(0x7FFFFFFF - mi);
    key = wave_max_u64(key);
    cnt = wave_sum_i32(cnt);
    const int wbad = __any(bad) ? 1 : 0;
    if (lane == 0) {
        s_key[w] = key;
        s_cnt[w] = cnt;
        s_bad[w] = wbad;
    }
    __syncthreads();
    // every lane takes one wave's entry and a butterfly over NW lanes finishes (maximum of an order, integer sum, OR: any tree gives the
    // same result); reading all NW entries per thread instead would hold 4 NW registers next to the row
    key = s_key[lane & (NW - 1)];
    cnt = s_cnt[lane & (NW - 1)];
    int anybad = s_bad[lane & (NW - 1)];
#pragma unroll
    for (int o = NW / 2; o > 0; o >>= 1) {
        const uint64_t y = (uint64_t)__shfl_xor((long long)key, o, 64);
        key = y > key ? y : key;
        cnt += __shfl_xor(cnt, o, 64);
        anybad |= __shfl_xor(anybad, o, 64);
    }
    const int amax = 0x7FFFFFFF - (int)(uint32_t)key;
    {
        const uint32_t kb = (uint32_t)(key >> 32);
        mx = __uint_as_float((kb & 0x80000000u) ? (kb & 0x7FFFFFFFu) : ~kb);
    }
    const bool row_bad = anybad != 0 || !(mx > -INFINITY);

    // ---- sweep 2: sum exp(x - max) over the same registers
    float se = 0.f;
    if (!row_bad) {
#pragma unroll
        for (int k = 0; k < nvec; ++k) {
            const f32x4 v = vec(k);
            se += (__expf(v[0] - mx) + __expf(v[1] - mx)) + (__expf(v[2] - mx) + __expf(v[3] - mx));
        }
        if (own_tail) {
            const f32x4 v = score_tail(row, V);
            se += (__expf(v[0] - mx) + __expf(v[1] - mx)) + __expf(v[2] - mx);
        }
    }
    se = wave_sum(se);
    if (lane == 0) s_sum[w] = se;
    __syncthreads();
    se = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) se += s_sum[i];
    const float qnan = __uint_as_float(0x7FC00000u);
    const float lg = logf(se);
    const float lse = row_bad ? qnan : mx + lg;

    if (tid == 0) {
        float lp;
        if (t < 0) lp = 0.f;
        else if (t >= V) lp = -INFINITY;
        else lp = row_bad ? qnan : (xt - mx) - lg;
        const bool scored = has_t && !row_bad;
        logprob[r] = lp;
        if (lse_out != nullptr) lse_out[r] = lse;
        argmax_out[r] = row_bad ? 0 : (int64_t)amax;
        greedy_out[r] = (scored && amax == ti) ? 1 : 0;
        if (rank_out != nullptr) rank_out[r] = scored ? cnt : -1;
        const int bits = (t >= V ? 1 : 0) | (row_bad ? 2 : 0);
        if (bits != 0 && status != nullptr) atomicOr(status, bits);
    }
    if (tid < n_cand) {
        const int64_t c = cand_ids[tid];
        cand_logprob[r * n_cand + tid] = (c >= 0 && c < V && !row_bad) ? row[c] - lse : qnan;
    }
}

// One wave per segment: sum_logprob[n] = the logprob values of rows [seg_start[n], seg_start[n + 1]) added ONE AFTER THE OTHER in row
// order, starting from 0 (64 values per coalesced load, then broadcast lane by lane: every lane does the same additions), so the result
// depends on the segment alone, not on N or the grid.  all_greedy[n] = every row of the segment is greedy (1 for an empty segment).
__global__ __launch_bounds__(64) void score_segments_kernel(const float* __restrict__ logprob, const uint8_t* __restrict__ greedy,
                                                            const int64_t* __restrict__ seg_start, int64_t rows,
                                                            float* __restrict__ sum_logprob, uint8_t* __restrict__ all_greedy) {
#pragma clang fp reassociate(off)
    const int64_t n = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t r0 = seg_start[n], r1 = seg_start[n + 1];
    r0 = r0 < 0 ? 0 : (r0 > rows ? rows : r0);  // device data: stay inside the arrays whatever it holds
    r1 = r1 < r0 ? r0 : (r1 > rows ? rows : r1);
    float acc = 0.f;
    bool ok = true;
    for (int64_t base = r0; base < r1; base += 64) {
        const int64_t i = base + lane;
        const float v = i < r1 ? logprob[i] : 0.f;
        const bool g = i < r1 ? greedy[i] != 0 : true;
        const int m = (int)(r1 - base < 64 ? r1 - base : 64);
        for (int j = 0; j < m; ++j) acc = acc + __shfl(v, j, 64);
        ok = ok && __all(g);
    }
    if (lane == 0) {
        sum_logprob[n] = acc;
        all_greedy[n] = ok ? 1 : 0;
    }
}

template <int THREADS, int NV>
static void launch_score(int64_t rows, hipStream_t s, const float* logits, int64_t ld, int V, const int64_t* targets, float* logprob, float* lse,
                         int64_t* argmax, uint8_t* greedy, int* rank, const int64_t* cand_ids, int n_cand, float* cand_logprob, int* status) {
    hipLaunchKernelGGL((score_rows_kernel<THREADS, NV>), dim3((unsigned)rows), dim3(THREADS), 0, s, logits, ld, V, targets, logprob, lse, argmax,
                       greedy, rank, cand_ids, n_cand, cand_logprob, status);
}

}  // namespace

extern "C" int dllm_score_rows(const float* logits, int64_t ld, int64_t rows, int V, const int64_t* targets, float* logprob, float* lse,
                               int64_t* argmax, void* greedy, int* rank, const int64_t* cand_ids, int n_cand, float* cand_logprob,
                               int* status, void* stream) {
    if (rows < 0 || rows > 0x7FFFFFFF || V <= 0 || V > (1 << 30) || ld < V || (ld & 3) || n_cand < 0 || n_cand > SCORE_MAX_CAND) return DLLM_ERR_SHAPE;
    if (logits == nullptr || targets == nullptr || logprob == nullptr || argmax == nullptr || greedy == nullptr) return DLLM_ERR_SHAPE;
    if (n_cand > 0 && (cand_ids == nullptr || cand_logprob == nullptr)) return DLLM_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(logits) & 15) return DLLM_ERR_ALIGN;
    if (rows == 0) return DLLM_OK;
    hipStream_t s = (hipStream_t)stream;
    auto* g = static_cast<uint8_t*>(greedy);
    if (V <= 1024)
        launch_score<256, 1>(rows, s, logits, ld, V, targets, logprob, lse, argmax, g, rank, cand_ids, n_cand, cand_logprob, status);
    else if (V <= 8192)
        launch_score<256, 8>(rows, s, logits, ld, V, targets, logprob, lse, argmax, g, rank, cand_ids, n_cand, cand_logprob, status);
    else if (V <= 32768)
        launch_score<1024, 8>(rows, s, logits, ld, V, targets, logprob, lse, argmax, g, rank, cand_ids, n_cand, cand_logprob, status);
    else
        launch_score<1024, 0>(rows, s, logits, ld, V, targets, logprob, lse, argmax, g, rank, cand_ids, n_cand, cand_logprob, status);
    return dllm_check_launch();
}

extern "C" int dllm_score_segments(const float* logprob, const void* greedy, const int64_t* seg_start, int64_t n_seg, int64_t rows,
                                   float* sum_logprob, void* all_greedy, void* stream) {
    if (n_seg < 0 || n_seg > 0x7FFFFFFF || rows < 0) return DLLM_ERR_SHAPE;
    if (n_seg == 0) return DLLM_OK;
    if (logprob == nullptr || greedy == nullptr || seg_start == nullptr || sum_logprob == nullptr || all_greedy == nullptr) return DLLM_ERR_SHAPE;
    hipLaunchKernelGGL(score_segments_kernel, dim3((unsigned)n_seg), dim3(64), 0, (hipStream_t)stream, logprob,
                       static_cast<const uint8_t*>(greedy), seg_start, rows, sum_logprob, static_cast<uint8_t*>(all_greedy));
    return dllm_check_launch();
}
