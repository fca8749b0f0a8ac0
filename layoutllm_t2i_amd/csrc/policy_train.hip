// The update of LayoutLLM-T2I's example-selection policy (train_rl.py:167-172, :85-95 and :182-184 of the reference): the REINFORCE loss
// of one rollout batch with its gradient to the policy layer, and one torch.optim.Adam step on that layer.  The reference builds the
// loss from two nn.Linear calls, a torch.mm, F.softmax and torch.log in fp32 and leaves the gradient to autograd.
//
//     q_p = W x_p + b            c_n = W y_n + b            z_pn = q_p . c_n / T
//     logpi_pn = z_pn - logsumexp_n(z_p,:)
//     logp_p   = sum_j logpi_{p, sel[p,j]}                  loss = - sum_p reward_p logp_p
//     G_pn     = -(reward_p / T) (m_pn - k_p pi_pn)         m_pn = times n occurs in sel[p,:], k_p = valid entries of sel[p,:]
//     dQ = G C       dC = G^T Q
//     grad_W = dQ^T X + dC^T Y       grad_b = sum_p dQ_p + sum_n dC_n
//
// G is d loss / d z: d logpi_pj / d z_pn = [n == j] - pi_pn, summed over the selected j and scaled by -reward_p; the 1 / T of
// z = q . c / T is folded into it.  An entry of sel outside [0, N) is skipped (it is not counted in k_p either), so no index read from
// device memory addresses outside the pool; a repeated index counts as often as it occurs, as the reference's loop over pool_ids does.
//
// The problem is small (the trainer: P <= 64 prompts, N = 32 candidates, D = 768, E = 128): four launches of plain vector code, all
// arithmetic in double from the fp32 operands, 64-lane butterfly sums, no atomics, every sum in an order fixed by the sizes alone --
// two calls on the same inputs give bit-equal outputs, and a prompt's logp does not depend on its row index.
//     policy_proj_kernel    R[r, e] = W[e, :] . row_r + b[e], rows = the P prompts then the N candidates     one wave per (r, e)
//     policy_row_kernel     one block per prompt: z_p,: (one wave per n), max / sum -> logsumexp, logp_p, the row of G
//     policy_back_kernel    dR[r, e]: dQ for the prompt rows, dC for the candidate rows                       one thread per (r, e)
//     policy_gradw_kernel   grad_W[e, d] over the P + N rows (one thread per (e, d)); grad_b[e] (one wave per e); the loss (one thread,
//                           p in index order) in the launch's last block
// The log-softmax is z - logsumexp(z): the reference's log(softmax(z)) in fp32 is -inf once a probability underflows, this form is
// finite for every finite z.  grad_W and grad_b are rounded to fp32 once.
//
// policy_adam_kernel: one elementwise launch over the E D + E elements of (W, bias), torch.optim.Adam with weight_decay = 0 and no
// amsgrad (the settings of train_rl.py:119) in torch's operation order (exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), the denominator
// sqrt(v) / sqrt(1 - beta2^step) + eps, addcdiv_ with lr / (1 - beta1^step)), each in double from the fp32 values, each stored value
// rounded to fp32 once.  The two bias corrections are computed on the host in double, as torch computes them in Python.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "common.h"
#include "gligen_hip.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_WAVES = PT_THREADS / 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
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
    for (int i = 1; i < PT_WAVES; ++i) out = is_max ? fmax(out, part[i]) : out + part[i];
    __syncthreads();
    return out;
}

// R[r, e] = W[e, :] . row_r + bias[e] in double, row_r = prompt[r] for r < P, cand[r - P] otherwise; one wave per (r, e)
__global__ __launch_bounds__(PT_THREADS) void policy_proj_kernel(const float* __restrict__ prompt, const float* __restrict__ cand,
                                                                  const float* __restrict__ W, const float* __restrict__ bias, int P, int N,
                                                                  int D, int E, double* __restrict__ R) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * PT_WAVES + (threadIdx.x >> 6);
    if (w >= (long long)(P + N) * E) return;
    const int r = (int)(w / E), e = (int)(w % E);
    const float4* x = reinterpret_cast<const float4*>(r < P ? prompt + (size_t)r * D : cand + (size_t)(r - P) * D);
    const float4* wr = reinterpret_cast<const float4*>(W + (size_t)e * D);
    double acc = 0.0;
    for (int i = lane; i < D / 4; i += 64) {
        const float4 a = x[i], b = wr[i];
        acc = fma((double)a.x, (double)b.x, acc);
        acc = fma((double)a.y, (double)b.y, acc);
        acc = fma((double)a.z, (double)b.z, acc);
        acc = fma((double)a.w, (double)b.w, acc);
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) R[(size_t)r * E + e] = acc + (double)bias[e];
}

// One block per prompt p.  G[p, :] first holds z_p,: = q_p . c_n / T, then the row of d loss / d z.  logp[p] is summed over sel[p, :] in
// index order by one thread.
__global__ __launch_bounds__(PT_THREADS) void policy_row_kernel(const double* __restrict__ R, const int32_t* __restrict__ sel,
                                                                 const double* __restrict__ reward, int P, int N, int E, int k,
                                                                 double temperature, double* __restrict__ G, double* __restrict__ logp) {
    __shared__ double q[GL_POLICY_MAX_DIM];
    __shared__ double part[PT_WAVES];
    __shared__ int32_t s[GL_POLICY_MAX_SHOTS];
    __shared__ int valid;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < E; e += PT_THREADS) q[e] = R[(size_t)p * E + e];
    if (tid < k) {
        const int32_t v = sel[(size_t)p * k + tid];
        s[tid] = (v >= 0 && v < N) ? v : -1;
    }
    __syncthreads();
    double* g = G + (size_t)p * N;
    const double* C = R + (size_t)P * E;
    for (int n = wave; n < N; n += PT_WAVES) {
        const double* c = C + (size_t)n * E;
        double acc = 0.0;
        for (int e = lane; e < E; e += 64) acc = fma(q[e], c[e], acc);
        acc = wave_sum_f64(acc);
        if (lane == 0) g[n] = acc / temperature;
    }
    __syncthreads();
    double m = -INFINITY;
    for (int n = tid; n < N; n += PT_THREADS) m = fmax(m, g[n]);
    m = block_reduce(m, true, part);
    double sum = 0.0;
    for (int n = tid; n < N; n += PT_THREADS) sum += exp(g[n] - m);
    sum = block_reduce(sum, false, part);
    const double lse = m + log(sum);
    if (tid == 0) {
        double lp = 0.0;
        int kp = 0;
        for (int j = 0; j < k; ++j)
            if (s[j] >= 0) {
                lp += g[s[j]] - lse;
                ++kp;
            }
        logp[p] = lp;
        valid = kp;
    }
    __syncthreads();                                   // z is read above, overwritten below
    const double scale = -reward[p] / temperature, kp = (double)valid;
    for (int n = tid; n < N; n += PT_THREADS) {
        int cnt = 0;
        for (int j = 0; j < k; ++j) cnt += s[j] == n ? 1 : 0;
        g[n] = scale * ((double)cnt - kp * exp(g[n] - lse));
    }
}

// dR[r, e]: r < P: dQ[p, e] = sum_n G[p, n] C[n, e]; otherwise n = r - P: dC[n, e] = sum_p G[p, n] Q[p, e]; one thread per (r, e)
__global__ __launch_bounds__(PT_THREADS) void policy_back_kernel(const double* __restrict__ R, const double* __restrict__ G, int P, int N,
                                                                  int E, double* __restrict__ dR) {
    const long long i = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= (long long)(P + N) * E) return;
    const int r = (int)(i / E), e = (int)(i % E);
    double acc = 0.0;
    if (r < P) {
        const double* g = G + (size_t)r * N;
        const double* C = R + (size_t)P * E;
        for (int n = 0; n < N; ++n) acc = fma(g[n], C[(size_t)n * E + e], acc);
    } else {
        const int n = r - P;
        for (int p = 0; p < P; ++p) acc = fma(G[(size_t)p * N + n], R[(size_t)p * E + e], acc);
    }
    dR[i] = acc;
}

// blocks [0, wblocks): grad_W[e, d] = sum_r dR[r, e] row_r[d], one thread per (e, d); blocks [wblocks, gridDim.x - 1): grad_b[e] =
// sum_r dR[r, e], one wave per e; the last block: loss = -sum_p reward[p] logp[p], p in index order
__global__ __launch_bounds__(PT_THREADS) void policy_gradw_kernel(const float* __restrict__ prompt, const float* __restrict__ cand,
                                                                   const double* __restrict__ dR, const double* __restrict__ reward,
                                                                   const double* __restrict__ logp, int P, int N, int D, int E, int wblocks,
                                                                   float* __restrict__ grad_W, float* __restrict__ grad_b,
                                                                   double* __restrict__ loss) {
    const int b = blockIdx.x;
    if (b == (int)gridDim.x - 1) {
        if (threadIdx.x == 0) {
            double acc = 0.0;
            for (int p = 0; p < P; ++p) acc = fma(reward[p], logp[p], acc);
            loss[0] = -acc;
        }
        return;
    }
    if (b >= wblocks) {
        const int e = (b - wblocks) * PT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (e >= E) return;                            // wave-uniform
        double acc = 0.0;
        for (int r = lane; r < P + N; r += 64) acc += dR[(size_t)r * E + e];
        acc = wave_sum_f64(acc);
        if (lane == 0) grad_b[e] = (float)acc;
        return;
    }
    const int i = b * PT_THREADS + threadIdx.x;
    if (i >= E * D) return;
    const int e = i / D, d = i % D;
    double acc = 0.0;
    for (int p = 0; p < P; ++p) acc = fma(dR[(size_t)p * E + e], (double)prompt[(size_t)p * D + d], acc);
    const double* dC = dR + (size_t)P * E;
    for (int n = 0; n < N; ++n) acc = fma(dC[(size_t)n * E + e], (double)cand[(size_t)n * D + d], acc);
    grad_W[i] = (float)acc;
}

// element i < nw: W; otherwise bias.  step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step)
__global__ __launch_bounds__(PT_THREADS) void policy_adam_kernel(float* __restrict__ W, float* __restrict__ bias, const float* __restrict__ gW,
                                                                  const float* __restrict__ gb, float* __restrict__ mW, float* __restrict__ vW,
                                                                  float* __restrict__ mb, float* __restrict__ vb, int nw, int nb, double beta1,
                                                                  double beta2, double step_size, double bc2_sqrt, double eps) {
    int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= nw + nb) return;
    float *p = W, *m = mW, *v = vW;
    const float* g = gW;
    if (i >= nw) {
        i -= nw;
        p = bias, m = mb, v = vb, g = gb;
    }
    const double gd = (double)g[i];
    double md = (double)m[i], vd = (double)v[i];
    md = md + (gd - md) * (1.0 - beta1);
    vd = beta2 * vd + (1.0 - beta2) * gd * gd;
    m[i] = (float)md;
    v[i] = (float)vd;
    p[i] = (float)((double)p[i] - step_size * (md / (sqrt(vd) / bc2_sqrt + eps)));
}

int refuse_as(const char* entry, const char* fmt, long long a0, long long a1) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a0, a1);
    gl_set_handleless_error((std::string(entry) + ": " + buf).c_str());
    return GL_ERR_BAD_ARG;
}
int refuse(const char* fmt, long long a0 = 0, long long a1 = 0) { return refuse_as("gl_policy_grad", fmt, a0, a1); }
int refuse_adam(const char* fmt, long long a0 = 0, long long a1 = 0) { return refuse_as("gl_policy_adam_step", fmt, a0, a1); }

constexpr int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// the scratch: R [P + N, E], G [P, N], dR [P + N, E], doubles
struct Carve {
    int64_t r, g, dr, total;
};

Carve carve(int64_t P, int64_t N, int64_t E) {
    Carve s;
    s.r = 0;
    s.g = s.r + align256((P + N) * E * 8);
    s.dr = s.g + align256(P * N * 8);
    s.total = s.dr + align256((P + N) * E * 8);
    return s;
}

bool sizes_ok(int64_t P, int64_t N, int64_t D, int64_t E, int64_t k) {
    return P >= 1 && P <= GL_POLICY_MAX_PROMPTS && N >= 1 && N <= GL_POLICY_TRAIN_MAX_CANDS && D >= 4 && D % 4 == 0 && D <= GL_POLICY_MAX_DIM &&
           E >= 1 && E <= GL_POLICY_MAX_DIM && k >= 1 && k <= GL_POLICY_MAX_SHOTS;
}

}  // namespace

extern "C" int64_t gl_policy_grad_scratch_bytes(int32_t P, int32_t N, int32_t D, int32_t E, int32_t k) {
    if (!sizes_ok(P, N, D, E, k)) return GL_ERR_BAD_ARG;
    return carve(P, N, E).total;
}

extern "C" int gl_policy_grad(const gl_policy_grad_args* a, void* stream) {
    if (!a) return refuse("null args");
    if (!a->prompt || !a->cand) return refuse("null input pointer (prompt / cand)");
    if (!a->W) return refuse("null W: the identity policy (add_linear=False) has nothing to train");
    if (!a->bias) return refuse("null input pointer (bias)");
    if (!a->sel || !a->reward) return refuse("null input pointer (sel / reward)");
    if (!a->loss || !a->logp || !a->grad_W || !a->grad_b) return refuse("null output pointer (loss / logp / grad_W / grad_b)");
    if (a->P < 1 || a->P > GL_POLICY_MAX_PROMPTS) return refuse("P = %lld outside [1, %lld]", a->P, GL_POLICY_MAX_PROMPTS);
    if (a->N < 1 || a->N > GL_POLICY_TRAIN_MAX_CANDS) return refuse("N = %lld outside [1, %lld]", a->N, GL_POLICY_TRAIN_MAX_CANDS);
    if (a->D < 4 || a->D % 4 != 0 || a->D > GL_POLICY_MAX_DIM) return refuse("D = %lld: need a multiple of 4 in [4, %lld]", a->D, GL_POLICY_MAX_DIM);
    if (a->E < 1 || a->E > GL_POLICY_MAX_DIM) return refuse("E = %lld outside [1, %lld]", a->E, GL_POLICY_MAX_DIM);
    if (a->k < 1 || a->k > GL_POLICY_MAX_SHOTS) return refuse("k = %lld outside [1, %lld]", a->k, GL_POLICY_MAX_SHOTS);
    if (!(a->temperature > 0.0)) return refuse("temperature must be > 0");
    const Carve s = carve(a->P, a->N, a->E);
    if (!a->scratch) return refuse("null scratch (needs %lld bytes)", s.total);
    if (a->scratch_bytes < s.total) return refuse("scratch of %lld bytes, needs %lld (gl_policy_grad_scratch_bytes)", a->scratch_bytes, s.total);
    if (((uintptr_t)a->prompt | (uintptr_t)a->cand | (uintptr_t)a->W | (uintptr_t)a->scratch) % 16 != 0)
        return refuse("prompt / cand / W / scratch must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(a->scratch);
    double* R = reinterpret_cast<double*>(base + s.r);
    double* G = reinterpret_cast<double*>(base + s.g);
    double* dR = reinterpret_cast<double*>(base + s.dr);
    const int P = a->P, N = a->N, D = a->D, E = a->E;
    const long long cells = (long long)(P + N) * E;                          // at most 4160 * 1024
    policy_proj_kernel<<<dim3((unsigned)((cells + PT_WAVES - 1) / PT_WAVES)), dim3(PT_THREADS), 0, st>>>(a->prompt, a->cand, a->W, a->bias, P, N, D, E, R);
    GL_CHECK_LAUNCH();
    policy_row_kernel<<<dim3(P), dim3(PT_THREADS), 0, st>>>(R, a->sel, a->reward, P, N, E, a->k, a->temperature, G, a->logp);
    GL_CHECK_LAUNCH();
    policy_back_kernel<<<dim3((unsigned)((cells + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, st>>>(R, G, P, N, E, dR);
    GL_CHECK_LAUNCH();
    const int wblocks = (E * D + PT_THREADS - 1) / PT_THREADS, bblocks = (E + PT_WAVES - 1) / PT_WAVES;
    policy_gradw_kernel<<<dim3(wblocks + bblocks + 1), dim3(PT_THREADS), 0, st>>>(a->prompt, a->cand, dR, a->reward, a->logp, P, N, D, E, wblocks,
                                                                                  a->grad_W, a->grad_b, a->loss);
    GL_CHECK_LAUNCH();
    return 0;
}
extern "C" int gl_sizeof_policy_grad_args(void) { return (int)sizeof(gl_policy_grad_args); }

extern "C" int gl_policy_adam_step(const gl_policy_adam_args* a, void* stream) {
    if (!a) return refuse_adam("null args");
    if (!a->W || !a->bias) return refuse_adam("null parameter pointer (W / bias)");
    if (!a->grad_W || !a->grad_b) return refuse_adam("null gradient pointer (grad_W / grad_b)");
    if (!a->exp_avg_W || !a->exp_avg_sq_W || !a->exp_avg_b || !a->exp_avg_sq_b) return refuse_adam("null state pointer (exp_avg / exp_avg_sq)");
    if (a->D < 4 || a->D % 4 != 0 || a->D > GL_POLICY_MAX_DIM) return refuse_adam("D = %lld: need a multiple of 4 in [4, %lld]", a->D, GL_POLICY_MAX_DIM);
    if (a->E < 1 || a->E > GL_POLICY_MAX_DIM) return refuse_adam("E = %lld outside [1, %lld]", a->E, GL_POLICY_MAX_DIM);
    if (a->step < 1) return refuse_adam("step = %lld: the step number after the increment, >= 1", a->step);
    if (!(a->lr >= 0.0) || isinf(a->lr)) return refuse_adam("lr must be finite and >= 0");
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0)) return refuse_adam("beta1 outside [0, 1)");
    if (!(a->beta2 >= 0.0 && a->beta2 < 1.0)) return refuse_adam("beta2 outside [0, 1)");
    if (!(a->eps >= 0.0) || isinf(a->eps)) return refuse_adam("eps must be finite and >= 0");
    const double bc1 = 1.0 - pow(a->beta1, (double)a->step), bc2 = 1.0 - pow(a->beta2, (double)a->step);
    const int nw = a->E * a->D, nb = a->E;
    policy_adam_kernel<<<dim3((nw + nb + PT_THREADS - 1) / PT_THREADS), dim3(PT_THREADS), 0, (hipStream_t)stream>>>(
        a->W, a->bias, a->grad_W, a->grad_b, a->exp_avg_W, a->exp_avg_sq_W, a->exp_avg_b, a->exp_avg_sq_b, nw, nb, a->beta1, a->beta2, a->lr / bc1,
        sqrt(bc2), a->eps);
    GL_CHECK_LAUNCH();
    return 0;
}
extern "C" int gl_sizeof_policy_adam_args(void) { return (int)sizeof(gl_policy_adam_args); }
