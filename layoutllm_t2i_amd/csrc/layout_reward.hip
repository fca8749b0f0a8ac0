// Layout terms of the RL rollout's reward (models/policy.py:126-135): tools/metrics.py:58-75 (maximum IoU per layout) and
// tools/metrics.py:93-144 (DocSim between two layouts), which the reference computes in CPU python with scipy's
// linear_sum_assignment, one Python call per box pair for DocSim.
//
// One 64-lane wave per (sample, term): grid = (B, 2), block = 64; term 0 = maximum IoU, term 1 = DocSim.  All arithmetic is
// double, uncontracted (the reference computes in float64 numpy).  A layout holds at most 64 boxes: one lane per column.
//
// Two accidents of the reference are kept:
//   * the same four numbers of a box are (l, t, r, b) to the IoU and (cx, cy, w, h) to DocSim (policy.py:130-134);
//   * the matrices are filled through np.meshgrid(range(n), range(m)) in its default 'xy' indexing and reshape(n, m), so flat
//     entry k holds f(box1[k % n], box2[k / n]): the transpose for n == m, a scrambled matrix for n != m.
//
// The assignment is solved by shortest augmenting paths (Jonker-Volgenant, as scipy's rectangular_lsap) on the negated
// matrix in LDS (64 x 64 doubles), transposed when it has more rows than columns: each lane owns one column (its dual, its
// path cost, its predecessor, its row) and one row (its dual, its column) in registers, the minimum over the open columns is
// a wave reduction.  Every loop is bounded: rows for the augmentations, columns for the path search, rows for the
// augmentation walk; no input can make the kernel spin.
//
// NaN: before the solver runs the wave checks its matrix (an IoU of two zero-area boxes is 0/0).  With any NaN entry the
// wave writes NaN for that term of that sample and skips the solver; the reference raises ValueError from scipy there
// ("matrix contains invalid numeric entries").  Infinite entries are not special-cased: a path search that finds no finite
// column (scipy: "cost matrix is infeasible") ends that term with NaN as well.
//
// It is a latency kernel: 2 B waves, a few KB of input, a dependent chain of wave reductions.  No roofline applies.
#include <math.h>
#include <stdio.h>
#include <string>

#include "common.h"
#include "gligen_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int LR_MAX = GL_LAYOUT_MAX_BOXES;
static_assert(LR_MAX == 64, "one lane per column");

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// compute_iou (metrics.py:29-42) of boxes read as (l, t, r, b)
__device__ __forceinline__ double box_iou(const double* p, const double* q) {
    const double l1 = p[0], t1 = p[1], r1 = p[2], b1 = p[3], l2 = q[0], t2 = q[1], r2 = q[2], b2 = q[3];
    const double a1 = (r1 - l1) * (b1 - t1), a2 = (r2 - l2) * (b2 - t2);
    const double l_max = fmax(l1, l2), r_min = fmin(r1, r2), t_max = fmax(t1, t2), b_min = fmin(b1, b2);
    const double ai = (l_max < r_min && t_max < b_min) ? (r_min - l_max) * (b_min - t_max) : 0.0;
    const double au = a1 + a2 - ai;
    return ai / au;
}

// __compute_bbox_sim (metrics.py:93-114) of boxes read as (cx, cy, w, h), C_S = 2, C = 0.5
__device__ __forceinline__ double box_sim(const double* p, const double* q) {
    const double dx = p[0] - q[0], dy = p[1] - q[1];
    const double delta_c = sqrt(dx * dx + dy * dy);
    const double delta_s = fabs(p[2] - q[2]) + fabs(p[3] - q[3]);
    const double area = fmin(p[2] * p[3], q[2] * q[3]);
    const double alpha = sqrt(area > 0.0 ? area : 0.0);
    return alpha * exp2(-1.0 * delta_c - 2.0 * delta_s);
}

// Minimum-cost assignment of the nr rows of cost[r * 64 + c] (nr <= nc <= 64) to distinct columns; returns the sum of the
// chosen entries, NaN when a path search finds no finite column.  Every value that steers control flow comes out of a wave
// reduction, a ballot or a broadcast, so the wave never diverges.
__device__ __forceinline__ double lsap_min(const double* cost, int nr, int nc, int lane) {
    double u = 0.0, v = 0.0;           // duals: u of row `lane`, v of column `lane`
    int col4row = -1, row4col = -1;    // column of row `lane`, row of column `lane`
    for (int cur = 0; cur < nr; ++cur) {
        double spc = INFINITY, min_val = 0.0;      // shortest path cost to column `lane`
        int path = -1, i = cur, sink = -1;
        bool SR = false, SC = false;
        for (int it = 0; it < nc && sink < 0; ++it) {          // each round closes one column
            i &= LR_MAX - 1;
            if (lane == i) SR = true;
            const double ui = __shfl(u, i, 64);
            const bool open = lane < nc && !SC;
            if (open) {
                const double r = min_val + cost[i * LR_MAX + lane] - ui - v;
                if (r < spc) {
                    spc = r;
                    path = i;
                }
            }
            const double lowest = wave_min_f64(open ? spc : (double)INFINITY);
            const unsigned long long tie = __ballot(open && spc == lowest);
            if (!(lowest < (double)INFINITY) || tie == 0) return NAN;
            // among equal columns an unassigned one ends the search (scipy's rule); then the lowest index
            const unsigned long long unassigned = __ballot(open && spc == lowest && row4col < 0);
            const int j = __ffsll((long long)(unassigned ? unassigned : tie)) - 1;
            min_val = lowest;
            const int r4c = __shfl(row4col, j, 64);
            if (lane == j) SC = true;
            if (r4c < 0) sink = j; else i = r4c;
        }
        if (sink < 0) return NAN;
        // dual update
        const double spc_of_my_col = __shfl(spc, col4row < 0 ? 0 : col4row, 64);
        if (lane == cur) u += min_val;
        else if (SR) u += min_val - spc_of_my_col;
        if (SC) v -= min_val - spc;
        // augment along the path back to `cur`
        int j = sink;
        for (int it = 0; it <= nr; ++it) {
            const int pi = __shfl(path, j, 64) & (LR_MAX - 1);
            if (lane == j) row4col = pi;
            const int prev = __shfl(col4row, pi, 64);
            if (lane == pi) col4row = j;
            if (pi == cur || prev < 0) break;
            j = prev;
        }
    }
    const double s = (lane < nr && col4row >= 0) ? cost[lane * LR_MAX + (col4row & (LR_MAX - 1))] : 0.0;
    return wave_sum_f64(s);
}

__global__ __launch_bounds__(64) void layout_reward_kernel(gl_layout_reward_args a) {
    __shared__ double cost[LR_MAX * LR_MAX];
    __shared__ double bg[LR_MAX][4], bp[LR_MAX][4];
    __shared__ int lg[LR_MAX], lp[LR_MAX], gi[LR_MAX], pj[LR_MAX];
    const int b = blockIdx.x, lane = threadIdx.x;
    // the host entry has validated the counts; the clamp keeps every index in range whatever the device copies hold
    const int N = min(max(a.n_gt[b], 0), LR_MAX), M = min(max(a.n_pred[b], 0), LR_MAX);
    const size_t row = (size_t)b * LR_MAX + lane;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bg[lane][c] = lane < N ? a.boxes_gt[row * 4 + c] : 0.0;
        bp[lane][c] = lane < M ? a.boxes_pred[row * 4 + c] : 0.0;
    }
    const int myg = lane < N ? a.labels_gt[row] : 0, myp = lane < M ? a.labels_pred[row] : 0;
    lg[lane] = myg;
    lp[lane] = myp;
    gi[lane] = 0;
    pj[lane] = 0;
    __syncthreads();

    if (blockIdx.y == 0) {
        // maximum IoU (metrics.py:58-75): per distinct ground-truth label, the best assignment of its boxes
        double score = 0.0;
        bool bad = false;
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int i = 0; i < N; ++i) {
            const int l = lg[i];
            if (__ballot(lane < i && myg == l)) continue;              // this label's group is done
            const unsigned long long mg = __ballot(lane < N && myg == l), mp = __ballot(lane < M && myp == l);
            const int n = __popcll(mg), m = __popcll(mp);
            if (m == 0) continue;
            __syncthreads();
            if ((mg >> lane) & 1ull) gi[__popcll(mg & below)] = lane;
            if ((mp >> lane) & 1ull) pj[__popcll(mp & below)] = lane;
            __syncthreads();
            bool nan = false;
            for (int k = lane; k < n * m; k += 64) {
                const double val = box_iou(bg[gi[k % n] & (LR_MAX - 1)], bp[pj[k / n] & (LR_MAX - 1)]);
                nan |= val != val;
                const int p = k / m, q = k % m;                        // reshape(n, m) of the flat fill
                cost[n <= m ? p * LR_MAX + q : q * LR_MAX + p] = -val;
            }
            __syncthreads();
            if (__ballot(nan)) {
                bad = true;
                break;
            }
            score -= lsap_min(cost, min(n, m), max(n, m), lane);
        }
        if (lane == 0) a.miou[b] = bad ? (double)NAN : score / (double)N;
    } else {
        // DocSim (metrics.py:116-144)
        double out = 0.0;
        if (!(N >= M + 3 || N <= M - 3) && N > 0 && M > 0) {
            bool nan = false;
            for (int k = lane; k < N * M; k += 64) {
                const int i1 = k % N, j2 = k / N;
                const double val = lg[i1] == lp[j2] ? box_sim(bg[i1], bp[j2]) : 0.0;
                nan |= val != val;
                const int p = k / M, q = k % M;
                cost[N <= M ? p * LR_MAX + q : q * LR_MAX + p] = -val;
            }
            __syncthreads();
            if (__ballot(nan)) out = NAN;
            else out = -lsap_min(cost, min(N, M), max(N, M), lane) / (double)min(N, M);
        }
        if (lane == 0) a.docsim[b] = out;
    }
}

thread_local std::string g_layout_err;

int refuse(const char* fmt, int a0 = 0, int a1 = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a0, a1);
    g_layout_err = std::string("gl_layout_reward: ") + buf;
    return GL_ERR_BAD_ARG;
}

}  // namespace

const char* gl_handleless_error() { return g_layout_err.c_str(); }
void gl_set_handleless_error(const char* msg) { g_layout_err = msg; }

extern "C" int gl_layout_reward(const gl_layout_reward_args* a, void* stream) {
    if (!a) return refuse("null args");
    if (!a->boxes_gt || !a->boxes_pred || !a->labels_gt || !a->labels_pred || !a->n_gt || !a->n_pred) return refuse("null device input pointer");
    if (!a->n_gt_host || !a->n_pred_host) return refuse("null host count array (n_gt_host / n_pred_host)");
    if (!a->miou || !a->docsim) return refuse("null output pointer");
    if (a->B < 1) return refuse("B = %d, need B >= 1", a->B);
    for (int b = 0; b < a->B; ++b) {
        const int n = a->n_gt_host[b], m = a->n_pred_host[b];
        if (n < 0 || n > LR_MAX) return refuse("n_gt[%d] = %d outside [0, 64]", b, n);
        if (m < 0 || m > LR_MAX) return refuse("n_pred[%d] = %d outside [0, 64]", b, m);
        if (n == 0) return refuse("n_gt[%d] = 0: an empty ground-truth layout (the reference divides by it)", b);
    }
    layout_reward_kernel<<<dim3(a->B, 2), dim3(64), 0, (hipStream_t)stream>>>(*a);
    GL_CHECK_LAUNCH();
    return 0;
}
extern "C" int gl_sizeof_layout_reward_args(void) { return (int)sizeof(gl_layout_reward_args); }
