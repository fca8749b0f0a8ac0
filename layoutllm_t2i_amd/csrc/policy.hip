// In-context example selection of LayoutLLM-T2I's policy (models/policy.py:11-33 with train_rl.py:167-172 / txt2img.py:472-474 and the
// ranking of txt2img.py:429): scores[p, n] = (W prompt_p + b) . (W cand_n + b), the k best candidates per prompt, optionally
// softmax(scores / temperature).  The reference runs two nn.Linear calls and a torch.mm in fp32 and ranks in Python on the host.
//
// The score is linear in the candidate, so the pool -- the large operand: 32 rows in the trainer, a whole caption file at inference --
// is never projected.  Per call
//     q_p = W prompt_p + b            policy_q_kernel      one wave per (p, e)
//     v_p = W^T q_p,  c_p = q_p . b   policy_fold_kernel   one thread per (p, d), one wave per p for c
//     scores[p, n] = v_p . cand_n + c_p                    policy_score_kernel
// The two small kernels (P E D and P D E multiply-adds, nothing beside the pool) sum in double and store v and c rounded to fp32 once,
// so the fold adds one rounding per element of v to the error of the fp32 dot product; the pool side is fp32 throughout.  The fold
// turns N D E multiply-adds into N D P and leaves the kernel bound by reading the N D 4 bytes of the pool.  With W == NULL
// (add_linear=False) v_p = prompt_p and c_p = 0, and the two small kernels are not launched.
//
// policy_score_kernel: one block of 4 waves per 64 consecutive candidate rows and per group of 8 prompts (grid.y); the group's
// vectors v sit in LDS ([min(P, 8)][D] fp32, at most 32 KiB).  A wave takes one row at a time: lane l holds the row's float4 l, l + 64, ...
// (16-byte loads, at most 4 per lane for D <= 1024), multiplies it into each v of the group with fmaf in a fixed order and sums the
// 64 partial sums with an xor butterfly.  No step depends on the row's index, on N or on the grid, so two equal rows get bit-equal
// scores and a permuted pool gives the permuted scores.  With P <= 8 the pool is read once; each further group of 8 prompts reads
// it again (the trainer's many-prompt calls have a 32-row pool).
//
// Top-k, two stages, no atomics, no flags: the ranking key of a score is the 64-bit word (monotone fp32 bits << 32) | ~index, so that
// a larger word is a better rank and equal scores rank the LOWER index first (the stable sorted(..., reverse=True) of txt2img.py:429).
// -0 ranks as +0 (Python compares them equal); a NaN gets the lowest score field, below -inf: the reference's order with a NaN among
// the scores is unspecified (Python's sort with an inconsistent comparison), here it is last, lower index first.  Stage one (the tail
// of policy_score_kernel): one lane per row of the block, a lane's rank is the count of better words among the 64, ranks below k are
// written to scratch [P, blocks, k].  Stage two (policy_merge_kernel, one block per prompt): k rounds, each the maximum of the words
// below the previous round's.  Words are distinct (the index is part of them), so the result does not depend on any order of execution.
//
// Probabilities (probs != NULL): softmax(scores / temperature) of train_rl.py:172.  A softmax of fp32 scores inherits their rounding times
// p (1 - p) / T, which at the rollout's temperatures is larger than the error of the reference's own fp32 softmax in some rows.  So the
// probabilities do not read the fp32 scores: policy_score_f64_kernel computes the scores once more in double (v and c unrounded; another
// read of the pool, paid only when probabilities are asked for: the trainer's pool has 32 rows) and policy_softmax_kernel (one block per
// prompt: max / sum / normalise over the [N] row) works in double and rounds each probability to fp32 once.  The scores output and
// the top-k are the fp32 path in either case, bit for bit.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "common.h"
#include "gligen_hip.h"

namespace {

constexpr int PB_ROWS = 64;        // candidate rows per block: one lane per row in the block-local ranking
constexpr int PB_GROUP = 8;        // prompts per block: their folded vectors in LDS
constexpr int PB_THREADS = 256;
static_assert(GL_POLICY_MAX_SHOTS < PB_ROWS, "every rank below k is taken by a lane");

typedef unsigned long long u64;

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// the ranking word of (score, index >= 0): never 0, which marks "no candidate"
__device__ __forceinline__ u64 rank_word(float s, int idx) {
    uint32_t key = 0;                                   // NaN: below every number
    if (s == s) {
        const uint32_t u = __float_as_uint(s + 0.0f);   // -0 -> +0
        key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((u64)key << 32) | (u64)(~(uint32_t)idx);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// q[p, e] = W[e, :] . prompt[p, :] + bias[e] in double; one wave per (p, e)
__global__ __launch_bounds__(PB_THREADS) void policy_q_kernel(const float* __restrict__ prompt, const float* __restrict__ W,
                                                               const float* __restrict__ bias, int P, int D, int E, double* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (PB_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= (long long)P * E) return;
    const int p = (int)(w / E), e = (int)(w % E);
    const float4* x = reinterpret_cast<const float4*>(prompt + (size_t)p * D);
    const float4* r = reinterpret_cast<const float4*>(W + (size_t)e * D);
    double acc = 0.0;
    for (int i = lane; i < D / 4; i += 64) {
        const float4 a = x[i], b = r[i];
        acc = fma((double)a.x, (double)b.x, acc);
        acc = fma((double)a.y, (double)b.y, acc);
        acc = fma((double)a.z, (double)b.z, acc);
        acc = fma((double)a.w, (double)b.w, acc);
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) q[(size_t)p * E + e] = acc + (double)bias[e];
}

// v[p, d] = sum_e W[e, d] q[p, e] (blocks x < gridDim.x - 1, one thread per d); c[p] = q[p, :] . bias (the last block's first wave);
// summed in double, stored as the fp32 values the score kernel reads and, when probabilities are asked for (vd != NULL), unrounded
__global__ __launch_bounds__(PB_THREADS) void policy_fold_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                                  const double* __restrict__ q, int D, int E, float* __restrict__ v,
                                                                  float* __restrict__ c, double* __restrict__ vd, double* __restrict__ cd) {
    const int p = blockIdx.y;
    const double* qp = q + (size_t)p * E;
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 64) {
            double acc = 0.0;
            for (int e = threadIdx.x; e < E; e += 64) acc = fma(qp[e], (double)bias[e], acc);
            acc = wave_sum_f64(acc);
            if (threadIdx.x == 0) {
                c[p] = (float)acc;
                if (cd) cd[p] = acc;
            }
        }
        return;
    }
    const int d = blockIdx.x * PB_THREADS + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int e = 0; e < E; ++e) acc = fma((double)W[(size_t)e * D + d], qp[e], acc);
    v[(size_t)p * D + d] = (float)acc;
    if (vd) vd[(size_t)p * D + d] = acc;
}

// The scores once more in double, for the probabilities only: sd[p, n] = v_p . cand_n + c_p with v, c unrounded (vd, cd; the identity:
// vf = the prompts, no c).  Same blocks as policy_score_kernel, groups of PB_GROUP64 prompts (their v in LDS as doubles, at most 32 KiB).
constexpr int PB_GROUP64 = 4;
__global__ __launch_bounds__(PB_THREADS) void policy_score_f64_kernel(const float* __restrict__ cand, const double* __restrict__ vd,
                                                                       const float* __restrict__ vf, const double* __restrict__ cd, int P,
                                                                       int N, int D, double* __restrict__ sd) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* vs = reinterpret_cast<double*>(smem);                            // [npg][D]
    const int D4 = D / 4;
    const int pg0 = blockIdx.y * PB_GROUP64, npg = min(PB_GROUP64, P - pg0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < npg * D; i += PB_THREADS) vs[i] = vd ? vd[(size_t)pg0 * D + i] : (double)vf[(size_t)pg0 * D + i];
    __syncthreads();
    const long long row0 = (long long)blockIdx.x * PB_ROWS;
    for (int r = wave; r < PB_ROWS; r += PB_THREADS / 64) {
        const long long n = row0 + r;
        if (n >= N) break;                                                   // wave-uniform
        const float4* x4 = reinterpret_cast<const float4*>(cand) + (size_t)n * D4;
        for (int p = 0; p < npg; ++p) {
            const double* w = vs + (size_t)p * D;
            double acc = 0.0;
            for (int i = lane; i < D4; i += 64) {
                const float4 x = x4[i];
                acc = fma((double)x.x, w[4 * i], acc);
                acc = fma((double)x.y, w[4 * i + 1], acc);
                acc = fma((double)x.z, w[4 * i + 2], acc);
                acc = fma((double)x.w, w[4 * i + 3], acc);
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) sd[(size_t)(pg0 + p) * N + (size_t)n] = acc + (cd ? cd[pg0 + p] : 0.0);
        }
    }
}

// NJ: float4 per lane and row, ceil(D / 256)
template <int NJ>
__global__ __launch_bounds__(PB_THREADS) void policy_score_kernel(const float* __restrict__ cand, const float* __restrict__ v,
                                                                   const float* __restrict__ c, int P, int N, int D, int k,
                                                                   float* __restrict__ scores, u64* __restrict__ local) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D4 = D / 4;
    const int pg0 = blockIdx.y * PB_GROUP, npg = min(PB_GROUP, P - pg0);
    const int gsz = min(PB_GROUP, P);                                                     // what the launch sized the LDS for
    float4* vs = reinterpret_cast<float4*>(smem);                                         // [gsz][D4]
    float* sc = reinterpret_cast<float*>(smem + (size_t)gsz * D4 * sizeof(float4));       // [gsz][PB_ROWS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float4* v4 = reinterpret_cast<const float4*>(v) + (size_t)pg0 * D4;
    for (int i = tid; i < npg * D4; i += PB_THREADS) vs[i] = v4[i];
    __syncthreads();

    const long long row0 = (long long)blockIdx.x * PB_ROWS;
    for (int r = wave; r < PB_ROWS; r += PB_THREADS / 64) {
        const long long n = row0 + r;
        if (n >= N) break;                                         // wave-uniform
        const float4* x4 = reinterpret_cast<const float4*>(cand) + (size_t)n * D4;
        float4 x[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = lane + 64 * j;
            x[j] = i < D4 ? x4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        for (int p = 0; p < npg; ++p) {
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = lane + 64 * j;
                if (i < D4) {
                    const float4 w = vs[p * D4 + i];
                    acc = fmaf(x[j].x, w.x, acc);
                    acc = fmaf(x[j].y, w.y, acc);
                    acc = fmaf(x[j].z, w.z, acc);
                    acc = fmaf(x[j].w, w.w, acc);
                }
            }
            acc = wave_sum_f32(acc);
            if (lane == 0) sc[p * PB_ROWS + r] = acc + (c ? c[pg0 + p] : 0.0f);
        }
    }
    __syncthreads();

    for (int i = tid; i < npg * PB_ROWS; i += PB_THREADS) {
        const int p = i / PB_ROWS, r = i % PB_ROWS;
        if (row0 + r < N) scores[(size_t)(pg0 + p) * N + (size_t)(row0 + r)] = sc[i];
    }
    if (k <= 0) return;
    // block-local ranking: lane = row; the rows past N carry the word 0 and rank after every candidate, by lane
    for (int p = wave; p < npg; p += PB_THREADS / 64) {
        const bool valid = row0 + lane < N;
        const u64 mine = valid ? rank_word(sc[p * PB_ROWS + lane], (int)(row0 + lane)) : 0ull;
        int rank = 0;
        for (int j = 0; j < PB_ROWS; ++j) {
            const u64 other = __shfl(mine, j, 64);
            rank += (other > mine || (other == mine && j < lane)) ? 1 : 0;
        }
        if (rank < k) local[((size_t)(pg0 + p) * gridDim.x + blockIdx.x) * k + rank] = mine;
    }
}

// topk[p, r] = index of the r-th best word of local[p, 0 .. M), -1 when fewer than r + 1 candidates exist; one block per prompt
__global__ __launch_bounds__(PB_THREADS) void policy_merge_kernel(const u64* __restrict__ local, long long M, int k, int32_t* __restrict__ topk) {
    __shared__ u64 part[PB_THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const u64* w = local + (size_t)p * M;
    u64 below = ~0ull;                                   // above every word: the score field of +inf is 0xFF800000, never all ones
    for (int r = 0; r < k; ++r) {
        u64 best = 0ull;
        for (long long i = tid; i < M; i += PB_THREADS) {
            const u64 x = w[i];
            if (x < below && x > best) best = x;
        }
        best = wave_max_u64(best);
        if ((tid & 63) == 0) part[tid >> 6] = best;
        __syncthreads();
        best = part[0];
#pragma unroll
        for (int i = 1; i < PB_THREADS / 64; ++i) best = part[i] > best ? part[i] : best;
        __syncthreads();
        if (tid == 0) topk[(size_t)p * k + r] = best ? (int32_t)(~(uint32_t)best) : -1;
        if (best == 0ull) {                              // block-uniform: nothing left
            for (int rr = r + 1 + tid; rr < k; rr += PB_THREADS) topk[(size_t)p * k + rr] = -1;
            return;
        }
        below = best;
    }
}

__device__ __forceinline__ double block_reduce(double v, bool is_max, double* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = is_max ? fmax(v, w) : v + w;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double out = part[0];
#pragma unroll
    for (int i = 1; i < PB_THREADS / 64; ++i) out = is_max ? fmax(out, part[i]) : out + part[i];
    __syncthreads();
    return out;
}

// probs[p, :] = softmax(sd[p, :] / temperature), computed in double and rounded to fp32 once; one block per prompt
__global__ __launch_bounds__(PB_THREADS) void policy_softmax_kernel(const double* __restrict__ sd, int N, double temperature,
                                                                     float* __restrict__ probs) {
    __shared__ double part[PB_THREADS / 64];
    const double* s = sd + (size_t)blockIdx.x * N;
    float* o = probs + (size_t)blockIdx.x * N;
    double m = -INFINITY;
    for (long long i = threadIdx.x; i < N; i += PB_THREADS) m = fmax(m, s[i] / temperature);
    m = block_reduce(m, true, part);
    double sum = 0.0;
    for (long long i = threadIdx.x; i < N; i += PB_THREADS) sum += exp(s[i] / temperature - m);
    sum = block_reduce(sum, false, part);
    for (long long i = threadIdx.x; i < N; i += PB_THREADS) o[i] = (float)(exp(s[i] / temperature - m) / sum);
}

int refuse(const char* fmt, long long a0 = 0, long long a1 = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a0, a1);
    gl_set_handleless_error((std::string("gl_policy_select: ") + buf).c_str());
    return GL_ERR_BAD_ARG;
}

constexpr int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

struct Carve {
    int64_t q, v, c, vd, cd, sd, local, total;
    long long blocks;
};

Carve carve(int64_t P, int64_t N, int64_t D, int64_t E, int64_t k, bool identity, bool probs) {
    Carve s;
    s.blocks = (N + PB_ROWS - 1) / PB_ROWS;
    s.q = 0;
    s.v = s.q + (identity ? 0 : align256(P * E * 8));
    s.c = s.v + (identity ? 0 : align256(P * D * 4));
    s.vd = s.c + (identity ? 0 : align256(P * 4));
    s.cd = s.vd + (identity || !probs ? 0 : align256(P * D * 8));
    s.sd = s.cd + (identity || !probs ? 0 : align256(P * 8));
    s.local = s.sd + (probs ? align256(P * N * 8) : 0);
    s.total = s.local + align256(P * s.blocks * k * 8);
    return s;
}

}  // namespace

extern "C" int64_t gl_policy_scratch_bytes(int32_t P, int32_t N, int32_t D, int32_t E, int32_t k, int32_t identity, int32_t probs) {
    if (P < 1 || N < 1 || D < 1 || E < 1 || k < 0) return GL_ERR_BAD_ARG;
    return carve(P, N, D, E, k, identity != 0, probs != 0).total;
}

extern "C" int gl_policy_select(const gl_policy_args* a, void* stream) {
    if (!a) return refuse("null args");
    if (!a->prompt || !a->cand) return refuse("null input pointer (prompt / cand)");
    if (a->W && !a->bias) return refuse("null bias with a weight matrix");
    if (!a->scores) return refuse("null output pointer (scores)");
    if (a->P < 1 || a->P > GL_POLICY_MAX_PROMPTS) return refuse("P = %lld outside [1, %lld]", a->P, GL_POLICY_MAX_PROMPTS);
    if (a->N < 1) return refuse("N = %lld, need N >= 1", a->N);
    if (a->D < 4 || a->D % 4 != 0 || a->D > GL_POLICY_MAX_DIM) return refuse("D = %lld: need a multiple of 4 in [4, %lld]", a->D, GL_POLICY_MAX_DIM);
    const bool identity = a->W == nullptr;
    if (a->E < 1 || a->E > GL_POLICY_MAX_DIM) return refuse("E = %lld outside [1, %lld]", a->E, GL_POLICY_MAX_DIM);
    if (identity && a->E != a->D) return refuse("E = %lld with W == NULL (the identity): need E == D = %lld", a->E, a->D);
    if (a->k < 0 || a->k > GL_POLICY_MAX_SHOTS) return refuse("k = %lld outside [0, %lld]", a->k, GL_POLICY_MAX_SHOTS);
    if (a->k > 0 && !a->topk) return refuse("null output pointer (topk) with k = %lld", a->k);
    if (a->probs && !(a->temperature > 0.0)) return refuse("temperature must be > 0 when probs is given");
    const Carve s = carve(a->P, a->N, a->D, a->E, a->k, identity, a->probs != nullptr);
    if (s.total > 0 && !a->scratch) return refuse("null scratch (needs %lld bytes)", s.total);
    if (a->scratch_bytes < s.total) return refuse("scratch of %lld bytes, needs %lld (gl_policy_scratch_bytes)", a->scratch_bytes, s.total);
    if (((uintptr_t)a->prompt | (uintptr_t)a->cand | (uintptr_t)a->W | (uintptr_t)a->scratch) % 16 != 0)
        return refuse("prompt / cand / W / scratch must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(a->scratch);
    const float* v = a->prompt;
    const float* c = nullptr;
    double* vd = nullptr;
    double* cd = nullptr;
    if (!identity) {
        double* q = reinterpret_cast<double*>(base + s.q);
        float* vv = reinterpret_cast<float*>(base + s.v);
        float* cc = reinterpret_cast<float*>(base + s.c);
        vd = a->probs ? reinterpret_cast<double*>(base + s.vd) : nullptr;
        cd = a->probs ? reinterpret_cast<double*>(base + s.cd) : nullptr;
        const long long waves = (long long)a->P * a->E;
        policy_q_kernel<<<dim3((unsigned)((waves + 3) / 4)), dim3(PB_THREADS), 0, st>>>(a->prompt, a->W, a->bias, a->P, a->D, a->E, q);
        GL_CHECK_LAUNCH();
        policy_fold_kernel<<<dim3((a->D + PB_THREADS - 1) / PB_THREADS + 1, a->P), dim3(PB_THREADS), 0, st>>>(a->W, a->bias, q, a->D, a->E, vv, cc, vd, cd);
        GL_CHECK_LAUNCH();
        v = vv;
        c = cc;
    }
    u64* local = reinterpret_cast<u64*>(base + s.local);
    const dim3 grid((unsigned)s.blocks, (a->P + PB_GROUP - 1) / PB_GROUP);
    const int gsz = a->P < PB_GROUP ? a->P : PB_GROUP;
    const size_t lds = (size_t)gsz * a->D * sizeof(float) + (size_t)gsz * PB_ROWS * sizeof(float);
    const int nj = (a->D / 4 + 63) / 64;
#define GL_POLICY_LAUNCH(NJ) \
    policy_score_kernel<NJ><<<grid, dim3(PB_THREADS), lds, st>>>(a->cand, v, c, a->P, a->N, a->D, a->k, a->scores, local)
    if (nj == 1) GL_POLICY_LAUNCH(1);
    else if (nj == 2) GL_POLICY_LAUNCH(2);
    else if (nj == 3) GL_POLICY_LAUNCH(3);
    else GL_POLICY_LAUNCH(4);
#undef GL_POLICY_LAUNCH
    GL_CHECK_LAUNCH();
    if (a->k > 0) {
        policy_merge_kernel<<<dim3(a->P), dim3(PB_THREADS), 0, st>>>(local, s.blocks * a->k, a->k, a->topk);
        GL_CHECK_LAUNCH();
    }
    if (a->probs) {
        double* sd = reinterpret_cast<double*>(base + s.sd);
        const int g64 = a->P < PB_GROUP64 ? a->P : PB_GROUP64;
        policy_score_f64_kernel<<<dim3((unsigned)s.blocks, (a->P + PB_GROUP64 - 1) / PB_GROUP64), dim3(PB_THREADS),
                                  (size_t)g64 * a->D * sizeof(double), st>>>(a->cand, vd, identity ? a->prompt : nullptr, cd, a->P, a->N, a->D, sd);
        GL_CHECK_LAUNCH();
        policy_softmax_kernel<<<dim3(a->P), dim3(PB_THREADS), 0, st>>>(sd, a->N, a->temperature, a->probs);
        GL_CHECK_LAUNCH();
    }
    return 0;
}
extern "C" int gl_sizeof_policy_args(void) { return (int)sizeof(gl_policy_args); }
