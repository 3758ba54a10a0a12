// Beam-search step of the decode loop: candidate selection, the hypothesis bookkeeping of transformers 4.35.2 [ext]
// `beam_search` + `BeamSearchScorer.process` and the update of the copy-free KV row map, in ONE launch per token step.
//
// Reference call site: omni/eval/vqa/vqa_inference.py:111-119 (`model.generate(num_beams=5, ...)` with `--beamsearch True`).
// The rules (INTEGRATION.md "Beam search"; restated in tests/beam_ref.py), for B batches of nb beams, row r = b * nb + beam:
//   1. s = log_softmax(logits[r][:V]) + beam_score[r] in fp32, as (x - max) - log(sum exp(x - max)) + beam_score.
//   2. per batch the top 2 nb of the nb * V scores, sorted descending; flat index = beam * V + id; ties: the lower flat index wins.
//   3. a batch that is not done walks its candidates in rank order: an eos candidate of rank < nb adds the hypothesis "parent's
//      tokens" with score s / (t + len_offset) ** length_penalty (double), t = tokens generated before it; an eos of rank >= nb is
//      skipped; any other candidate becomes the next running beam (score, token, parent) until nb are filled.  A full hypothesis
//      set admits a score above its worst and drops its lowest score (the earliest added on ties).  Then done |= is_done(top
//      candidate score, t + len_offset) (early_stopping 0 = False, 1 = True, 2 = "never" with max_new as the length when lp > 0).
//   4. a batch that is done emits pad with score 0 and parent = its beam 0.
//   5. non-finite rows (a NaN, or no finite maximum) set status[r] = 1 and their candidates rank as -inf.
//
// Form: one 512-thread block per row.  Each thread streams its strided ids once, keeping an online (max, sum exp) pair and a
// sorted top-K list of 64-bit keys (order-preserving fp32 key << 32 | ~id: a larger key is a larger logit, then a lower id) in
// registers; the block's top 2 nb come from 2 nb rounds of a block max over the list heads (the order within a row is the same for
// logits and log-probabilities).  Every float reduction has a fixed order: bit-identical launches.  The row publishes its 2 nb
// candidates (agent-scope release, arrival counter per batch); the last row of a batch to arrive merges the nb x 2 nb candidates in
// one wave, runs rule 3 on one thread, writes the beams, and permutes the batch's KV row map: map[r][0..c] = map[parent(r)][0..c]
// and map[r][c + 1] = r (c = kv_len - 1, the slot of the token whose logits these are).  Each thread owns whole map columns, so
// the in-place permutation needs no barrier: a column of all nb rows is read into registers, then written.  The last merge of the
// launch advances *step.
#include <cstring>

#include "common.h"

namespace {

constexpr int BEAM_THREADS = 512;
constexpr int BEAM_WAVES = BEAM_THREADS / 64;
constexpr int BEAM_MAX_NB = 8;

struct BeamArgs {
    const float* logits;
    int64_t ld;
    int B, nb, V;
    float* beam_score;
    int64_t* tok_out;
    int* parents;
    int64_t* tokens;
    int64_t n_steps;
    int64_t* step;
    int* arrive;
    float* ws_score;
    int* ws_flat;
    double* hyp_score;
    int* hyp_meta;  // [B * nb][3]: end step, end row, length
    int* hyp_count;
    double* worst;
    int* done;
    int64_t eos, pad;
    double lp;
    int early, max_new, len_offset;
    const int* kv_len;
    int* row_map;
    int64_t map_ld;
    float* cand_score;
    int* cand_flat;
    int* status;
};

__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ uint64_t pack(float v, uint32_t idx) { return ((uint64_t)f2key(v) << 32) | (0xFFFFFFFFu - idx); }
__device__ __forceinline__ uint32_t unpack_idx(uint64_t k) { return 0xFFFFFFFFu - (uint32_t)k; }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((unsigned int)v, o, 64), hi = __shfl_xor((unsigned int)(v >> 32), o, 64);
        const uint64_t y = ((uint64_t)hi << 32) | lo;
        v = y > v ? y : v;
    }
    return v;
}

// (max, sum exp(x - max)) pairs: b merged into a
__device__ __forceinline__ void lse_merge(float& m, float& s, float bm, float bsum) {
    const float mn = fmaxf(m, bm);
    if (mn == -INFINITY) return;
    s = s * expf(m - mn) + bsum * expf(bm - mn);
    m = mn;
}

__device__ void add_hypothesis(const BeamArgs& a, int bt, double score, int end_step, int end_row, int len, int& cnt, double& worst) {
    const int nb = a.nb;
    double* hs = a.hyp_score + (int64_t)bt * nb;
    int* hm = a.hyp_meta + (int64_t)bt * nb * 3;
    if (cnt < nb) {
        hs[cnt] = score;
        hm[cnt * 3 + 0] = end_step;
        hm[cnt * 3 + 1] = end_row;
        hm[cnt * 3 + 2] = len;
        ++cnt;
        worst = fmin(worst, score);
        return;
    }
    if (!(score > worst)) return;
    int wi = 0;  // the lowest score, the earliest added on ties (python's sorted() over (score, index))
    for (int i = 1; i < nb; ++i)
        if (hs[i] < hs[wi]) wi = i;
    for (int i = wi; i + 1 < nb; ++i) {  // delete it (the others keep their order), append the new one
        hs[i] = hs[i + 1];
        hm[i * 3 + 0] = hm[i * 3 + 3];
        hm[i * 3 + 1] = hm[i * 3 + 4];
        hm[i * 3 + 2] = hm[i * 3 + 5];
    }
    hs[nb - 1] = score;
    hm[(nb - 1) * 3 + 0] = end_step;
    hm[(nb - 1) * 3 + 1] = end_row;
    hm[(nb - 1) * 3 + 2] = len;
    double w = hs[0];
    for (int i = 1; i < nb; ++i) w = fmin(w, hs[i]);
    worst = w;
}

template <int K>
__global__ __launch_bounds__(BEAM_THREADS) void beam_step_kernel(BeamArgs a) {
    __shared__ uint64_t s_key[BEAM_WAVES];
    __shared__ float s_m[BEAM_WAVES], s_s[BEAM_WAVES];
    __shared__ int s_flag, s_last;
    __shared__ float s_cs[2 * BEAM_MAX_NB];
    __shared__ int s_cf[2 * BEAM_MAX_NB];
    __shared__ int n_par[BEAM_MAX_NB];
    __shared__ int64_t n_tok[BEAM_MAX_NB];
    __shared__ float n_score[BEAM_MAX_NB];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nb = a.nb, C = 2 * nb, bt = row / nb, beam = row % nb, V = a.V;
    const int64_t st = *a.step;        // read before this block's ticket: the launch's last merge advances it
    const float bsc = a.beam_score[row];  // read before the ticket: the batch's merge rewrites it
    if (tid == 0) s_flag = 0;
    __syncthreads();

    // ---- one pass over the row: online (max, sum exp) and the thread's top K
    uint64_t lst[K];
#pragma unroll
    for (int j = 0; j < K; ++j) lst[j] = 0;
    float m = -INFINITY, s = 0.f;
    bool nan = false;
    const float* x = a.logits + (int64_t)row * a.ld;
    for (int i = tid; i < V; i += BEAM_THREADS) {
        const float v = x[i];
        if (v != v) {
            nan = true;
            continue;
        }
        const uint64_t k = pack(v, (uint32_t)i);
        if (k > lst[K - 1]) {
#pragma unroll
            for (int j = K - 1; j > 0; --j) {
                const uint64_t lo = lst[j - 1] < k ? lst[j - 1] : k;
                lst[j] = lst[j] > lo ? lst[j] : lo;
            }
            lst[0] = lst[0] > k ? lst[0] : k;
        }
        if (v > m) {
            s = s * expf(m - v) + 1.f;
            m = v;
        } else if (v > -INFINITY) {
            s += expf(v - m);
        }
    }
    if (nan) atomicOr(&s_flag, 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float bm = __shfl_xor(m, o, 64), bs = __shfl_xor(s, o, 64);
        lse_merge(m, s, bm, bs);
    }
    if (lane == 0) {
        s_m[w] = m;
        s_s[w] = s;
    }
    __syncthreads();
    float M = s_m[0], S = s_s[0];
#pragma unroll
    for (int i = 1; i < BEAM_WAVES; ++i) lse_merge(M, S, s_m[i], s_s[i]);
    const bool bad = s_flag != 0 || !(fabsf(M) <= 3.402823466e38f);
    const float logsum = logf(S);

    // ---- the row's top 2 nb: 2 nb rounds of a block max over the list heads (keys are unique: distinct ids)
    float* wss = a.ws_score + (int64_t)row * C;
    int* wsf = a.ws_flat + (int64_t)row * C;
    for (int r = 0; r < C; ++r) {
        const uint64_t h = wave_max_u64(lst[0]);
        if (lane == 0) s_key[w] = h;
        __syncthreads();
        uint64_t best = s_key[0];
#pragma unroll
        for (int i = 1; i < BEAM_WAVES; ++i) best = s_key[i] > best ? s_key[i] : best;
        __syncthreads();
        if (best != 0 && lst[0] == best) {
#pragma unroll
            for (int j = 0; j < K - 1; ++j) lst[j] = lst[j + 1];
            lst[K - 1] = 0;
        }
        if (tid == 0) {
            const uint32_t id = bad ? (uint32_t)r : unpack_idx(best);
            wss[r] = bad ? -INFINITY : ((key2f((uint32_t)(best >> 32)) - M) - logsum) + bsc;
            wsf[r] = beam * V + (int)id;
        }
    }
    if (tid == 0 && bad) a.status[row] = 1;

    // ---- publish (agent-scope release) and draw a ticket; the batch's last row merges
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(a.arrive + bt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == nb - 1 ? 1 : 0;
        if (t == nb - 1) {
            __hip_atomic_store(a.arrive + bt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;

    // ---- merge: the batch's top 2 nb of nb x 2 nb candidates in wave 0
    const int base = bt * nb;
    if (w == 0) {
        const int n = nb * C;  // <= 128
        uint64_t k0 = 0, k1 = 0;
        if (lane < n) k0 = pack(a.ws_score[(int64_t)base * C + lane], (uint32_t)a.ws_flat[(int64_t)base * C + lane]);
        if (lane + 64 < n) k1 = pack(a.ws_score[(int64_t)base * C + lane + 64], (uint32_t)a.ws_flat[(int64_t)base * C + lane + 64]);
        for (int r = 0; r < C; ++r) {
            const uint64_t mine = k0 > k1 ? k0 : k1;
            const uint64_t best = wave_max_u64(mine);
            if (k0 == best) k0 = 0;
            else if (k1 == best) k1 = 0;
            if (lane == 0) {
                s_cs[r] = key2f((uint32_t)(best >> 32));
                s_cf[r] = (int)unpack_idx(best);
            }
        }
    }
    __syncthreads();

    // ---- rule 3 on one thread
    if (tid == 0) {
        int cnt = a.hyp_count[bt];
        double worst = a.worst[bt];
        int dn = a.done[bt];
        const int glen = (int)st + a.len_offset;
        int k = 0;
        if (!dn) {
            for (int r = 0; r < C && k < nb; ++r) {
                const int flat = s_cf[r], bm = flat / V, id = flat - bm * V;
                if (a.eos >= 0 && (int64_t)id == a.eos) {
                    if (r >= nb) continue;
                    const double sc = (double)s_cs[r] / pow((double)glen, a.lp);
                    add_hypothesis(a, bt, sc, (int)st, base + bm, (int)st, cnt, worst);
                } else {
                    n_score[k] = s_cs[r];
                    n_tok[k] = id;
                    n_par[k] = base + bm;
                    ++k;
                }
            }
            bool d = false;
            if (cnt >= nb) {
                if (a.early == 1) {
                    d = true;
                } else {
                    const double den = (a.early == 2 && a.lp > 0.0) ? (double)a.max_new : (double)glen;
                    d = worst >= (double)s_cs[0] / pow(den, a.lp);
                }
            }
            a.hyp_count[bt] = cnt;
            a.worst[bt] = worst;
            a.done[bt] = d ? 1 : 0;
        }
        for (; k < nb; ++k) {  // a done batch (k == 0); never more than nb eos among 2 nb candidates otherwise
            n_score[k] = dn ? 0.f : -INFINITY;
            n_tok[k] = a.pad;
            n_par[k] = base;
        }
        if (a.cand_score != nullptr) {
            for (int r = 0; r < C; ++r) {
                a.cand_score[(int64_t)bt * C + r] = s_cs[r];
                a.cand_flat[(int64_t)bt * C + r] = s_cf[r];
            }
        }
    }
    __syncthreads();
    const bool in_range = st >= 0 && st < a.n_steps;
    if (tid < nb) {
        const int r = base + tid;
        a.tok_out[r] = n_tok[tid];
        a.beam_score[r] = n_score[tid];
        if (in_range) {
            a.parents[st * a.B * nb + r] = n_par[tid];
            a.tokens[st * a.B * nb + r] = n_tok[tid];
        }
    }
    // ---- copy-free KV cache: the batch's row map follows the parents (each thread owns whole columns)
    if (a.row_map != nullptr) {
        const int c = a.kv_len[base] - 1;
        int* mp = a.row_map + (int64_t)base * a.map_ld;
        const int ncol = (int)min((int64_t)c + 1, a.map_ld);
        int src[BEAM_MAX_NB];
#pragma unroll
        for (int j = 0; j < BEAM_MAX_NB; ++j) src[j] = j < nb ? n_par[j] - base : j;
        for (int col = tid; col < ncol; col += BEAM_THREADS) {
            int v[BEAM_MAX_NB];
#pragma unroll
            for (int j = 0; j < BEAM_MAX_NB; ++j) v[j] = (j < nb && src[j] != j) ? mp[(int64_t)src[j] * a.map_ld + col] : 0;
#pragma unroll
            for (int j = 0; j < BEAM_MAX_NB; ++j)
                if (j < nb && src[j] != j) mp[(int64_t)j * a.map_ld + col] = v[j];
        }
        if (tid < nb && c >= -1 && (int64_t)c + 1 < a.map_ld) mp[(int64_t)tid * a.map_ld + c + 1] = base + tid;
    }
    // ---- the launch's last merge advances the step (every block read *step before its batch ticket)
    if (tid == 0) {
        const int t = __hip_atomic_fetch_add(a.arrive + a.B, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == a.B - 1) {
            __hip_atomic_store(a.arrive + a.B, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *a.step = st + 1;
        }
    }
}

}  // namespace

extern "C" int dllm_beam_step(const float* logits, int64_t ld, int B, int nb, int V, float* beam_score, int64_t* tok_out, int* parents,
                              int64_t* tokens, int64_t n_steps, int64_t* step, int* arrive, void* ws, double* hyp_score, int* hyp_meta,
                              int* hyp_count, double* worst, int* done, int64_t eos, int64_t pad, int64_t length_penalty_bits,
                              int early_stopping, int max_new, int len_offset, const int* kv_len, int* row_map, int64_t map_ld,
                              float* cand_score, int* cand_flat, int* status, void* stream) {
    if (B < 0 || nb < 1 || nb > BEAM_MAX_NB || V < 2 * nb || ld < V || (int64_t)nb * V > 0x7FFFFFFFLL || n_steps < 0)
        return DLLM_ERR_SHAPE;
    if (logits == nullptr || beam_score == nullptr || tok_out == nullptr || step == nullptr || arrive == nullptr || ws == nullptr ||
        hyp_score == nullptr || hyp_meta == nullptr || hyp_count == nullptr || worst == nullptr || done == nullptr || status == nullptr)
        return DLLM_ERR_SHAPE;
    if ((n_steps > 0 && (parents == nullptr || tokens == nullptr)) || (row_map != nullptr && (kv_len == nullptr || map_ld < 1)) ||
        (cand_score == nullptr) != (cand_flat == nullptr) || early_stopping < 0 || early_stopping > 2 || len_offset < 0)
        return DLLM_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(hyp_score) & 7 || reinterpret_cast<uintptr_t>(worst) & 7) return DLLM_ERR_ALIGN;
    if (B == 0) return DLLM_OK;
    BeamArgs a;
    a.logits = logits;
    a.ld = ld;
    a.B = B;
    a.nb = nb;
    a.V = V;
    a.beam_score = beam_score;
    a.tok_out = tok_out;
    a.parents = parents;
    a.tokens = tokens;
    a.n_steps = n_steps;
    a.step = step;
    a.arrive = arrive;
    a.ws_score = static_cast<float*>(ws);
    a.ws_flat = reinterpret_cast<int*>(static_cast<float*>(ws) + (int64_t)B * nb * 2 * nb);
    a.hyp_score = hyp_score;
    a.hyp_meta = hyp_meta;
    a.hyp_count = hyp_count;
    a.worst = worst;
    a.done = done;
    a.eos = eos;
    a.pad = pad;
    double lp;
    memcpy(&lp, &length_penalty_bits, sizeof(lp));
    a.lp = lp;
    a.early = early_stopping;
    a.max_new = max_new;
    a.len_offset = len_offset;
    a.kv_len = kv_len;
    a.row_map = row_map;
    a.map_ld = map_ld;
    a.cand_score = cand_score;
    a.cand_flat = cand_flat;
    a.status = status;
    const dim3 g((unsigned)(B * nb)), blk(BEAM_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (2 * nb <= 2)
        hipLaunchKernelGGL(beam_step_kernel<2>, g, blk, 0, s, a);
    else if (2 * nb <= 4)
        hipLaunchKernelGGL(beam_step_kernel<4>, g, blk, 0, s, a);
    else if (2 * nb <= 8)
        hipLaunchKernelGGL(beam_step_kernel<8>, g, blk, 0, s, a);
    else
        hipLaunchKernelGGL(beam_step_kernel<16>, g, blk, 0, s, a);
    return dllm_check_launch();
}
