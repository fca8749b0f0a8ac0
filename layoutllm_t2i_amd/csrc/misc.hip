// Small kernels of the denoising path: grounding-token input (Fourier box embedding + null blend),
// sinusoidal timestep embedding, SiLU, the PLMS/CFG latent update, latent packing, ABI introspection.
#include "common.h"
#include "gligen_hip.h"
#include "opts.h"

#include <initializer_list>

namespace {

// text_grounding_net.py:30-41 + util.py:12-26.  One block per (b, i) row; out row = [in_dim | 8*num_freqs].
// Fourier order: for each frequency f_j = 100^(j/num_freqs): sin(f_j * xyxy) (4) then cos(f_j * xyxy) (4).
// OT = half_t (default) or float (strict mode: the row is split into [hi | lo] by gl_split_f32 afterwards)
template <typename OT>
__global__ __launch_bounds__(256) void posnet_input_kernel(const float* __restrict__ boxes, const float* __restrict__ masks,
                                                           const float* __restrict__ emb, const float* __restrict__ null_pos,
                                                           const float* __restrict__ null_xyxy, int in_dim, int num_freqs,
                                                           OT* __restrict__ out) {
    const int row = blockIdx.x;
    const float m = masks[row];
    const int pos_dim = num_freqs * 8;
    OT* o = out + (size_t)row * (in_dim + pos_dim);
    for (int c = threadIdx.x; c < in_dim; c += 256) {
        const float v = emb[(size_t)row * in_dim + c] * m + (1.0f - m) * null_pos[c];
        o[c] = (OT)v;
    }
    for (int c = threadIdx.x; c < pos_dim; c += 256) {
        const int j = c / 8;
        const int r = c - j * 8;
        const int coord = r & 3;
        const float freq = powf(100.0f, (float)j / (float)num_freqs);
        const float arg = freq * boxes[(size_t)row * 4 + coord];
        const float e = (r < 4) ? sinf(arg) : cosf(arg);
        o[in_dim + c] = (OT)(e * m + (1.0f - m) * null_xyxy[c]);
    }
}

// text_image_grounding_net.py:48-61.  One block per (b, i) row writes BOTH MLP inputs: out_text row = [text_blend | xyxy_blend], out_image row =
// [image_blend | xyxy_blend].  The Fourier part is computed once and blended with masks; the embeddings are blended with text_masks /
// image_masks against their own null features (the operation order of :56-58).
template <typename OT>
__global__ __launch_bounds__(256) void posnet_input_ti_kernel(const float* __restrict__ boxes, const float* __restrict__ masks,
                                                              const float* __restrict__ text_masks, const float* __restrict__ image_masks,
                                                              const float* __restrict__ text_emb, const float* __restrict__ image_emb,
                                                              const float* __restrict__ null_text, const float* __restrict__ null_image,
                                                              const float* __restrict__ null_xyxy, int in_dim, int num_freqs,
                                                              OT* __restrict__ out_text, OT* __restrict__ out_image) {
    const int row = blockIdx.x;
    const float m = masks[row], tm = text_masks[row], im = image_masks[row];
    const int pos_dim = num_freqs * 8;
    OT* ot = out_text + (size_t)row * (in_dim + pos_dim);
    OT* oi = out_image + (size_t)row * (in_dim + pos_dim);
    for (int c = threadIdx.x; c < in_dim; c += 256) {
        ot[c] = (OT)(text_emb[(size_t)row * in_dim + c] * tm + (1.0f - tm) * null_text[c]);
        oi[c] = (OT)(image_emb[(size_t)row * in_dim + c] * im + (1.0f - im) * null_image[c]);
    }
    for (int c = threadIdx.x; c < pos_dim; c += 256) {
        const int j = c / 8;
        const int r = c - j * 8;
        const int coord = r & 3;
        const float freq = powf(100.0f, (float)j / (float)num_freqs);
        const float arg = freq * boxes[(size_t)row * 4 + coord];
        const float e = (r < 4) ? sinf(arg) : cosf(arg);
        const OT v = (OT)(e * m + (1.0f - m) * null_xyxy[c]);
        ot[in_dim + c] = v;
        oi[in_dim + c] = v;
    }
}

// keypoint_grounding_net.py:39-56 + util.py:12-26.  One block per (b, t) token row, t in [0, tokens = 17 P): person t / 17, keypoint t % 17.
// out row (ld columns, ld = D + 4 F rounded up to 64) = [ (person_emb[t / 17] + keypoint_emb[t % 17]) * m + (1 - m) * null_person  (D)
//                                                        | fourier(point) * m + (1 - m) * null_xy                                (4 F)
//                                                        | 0 (the pad columns of the padded-K linears.0, written here)          ]
// in fp32, the table sum first and then the blend, as the reference orders them; m is a blend factor (any value), not a select.
// Fourier order: for each frequency f_j = 100^(j/num_freqs): sin(f_j x), sin(f_j y), cos(f_j x), cos(f_j y).
template <typename OT>
__global__ __launch_bounds__(256) void posnet_input_kp_kernel(const float* __restrict__ points, const float* __restrict__ masks,
                                                              const float* __restrict__ person_emb, const float* __restrict__ keypoint_emb,
                                                              const float* __restrict__ null_person, const float* __restrict__ null_xy, int tokens,
                                                              int D, int num_freqs, int ld, OT* __restrict__ out) {
    const int row = blockIdx.x;
    const int t = row % tokens;
    const float m = masks[row];
    const int pos_dim = num_freqs * 4;
    const float* pe = person_emb + (size_t)(t / 17) * D;
    const float* ke = keypoint_emb + (size_t)(t % 17) * D;
    OT* o = out + (size_t)row * ld;
    for (int c = threadIdx.x; c < D; c += 256) {
        const float s = pe[c] + ke[c];
        o[c] = (OT)(s * m + (1.0f - m) * null_person[c]);
    }
    for (int c = threadIdx.x; c < pos_dim; c += 256) {
        const int j = c / 4;
        const int r = c - j * 4;
        const float freq = powf(100.0f, (float)j / (float)num_freqs);
        const float arg = freq * points[(size_t)row * 2 + (r & 1)];
        const float e = (r < 2) ? sinf(arg) : cosf(arg);
        o[D + c] = (OT)(e * m + (1.0f - m) * null_xy[c]);
    }
    for (int c = D + pos_dim + threadIdx.x; c < ld; c += 256) o[c] = (OT)0.0f;
}

// interface.py:126-129: out = norm * (f P) / || f P ||_2 per image, fp32.  f [n, dim], P [dim, dim] row-major (project(feature, P.T) =
// feature @ P), one block of 256 threads per image, dim <= 1024: thread t owns output columns t, t + 256, ... (coalesced reads of P's rows).
// Deliberately one block per image, so a single image streams all of P (2.4 MB at dim 768) through one CU: this runs once per distinct
// reference image at conditioning time, behind a CLIP vision forward that costs orders of magnitude more.
__global__ __launch_bounds__(256) void image_ground_feature_kernel(const float* __restrict__ feat, const float* __restrict__ proj, int dim,
                                                                   float norm, float* __restrict__ out) {
    __shared__ float f[1024];
    __shared__ float red[4];
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < dim; c += 256) f[c] = feat[(size_t)b * dim + c];
    __syncthreads();
    // two-level sum over k (chunks of 32, then the chunk sums): the rounding error grows with sqrt(32) + sqrt(dim / 32) instead of sqrt(dim)
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < dim; k0 += 32) {
        float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int k1 = k0 + 32 < dim ? k0 + 32 : dim;
        for (int k = k0; k < k1; ++k) {
            const float fk = f[k];
            const float* pr = proj + (size_t)k * dim;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = threadIdx.x + j * 256;
                if (c < dim) part[j] += fk * pr[c];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += part[j];
    }
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) ss += acc[j] * acc[j];       // (columns >= dim hold 0)
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float inv = norm / sqrtf(red[0] + red[1] + red[2] + red[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = threadIdx.x + j * 256;
        if (c < dim) out[(size_t)b * dim + c] = acc[j] * inv;
    }
}

// util.py:161-181: [cos(t*w) | sin(t*w)], w_k = exp(-ln(10000) * k / half)
template <typename OT>
__global__ void timestep_embedding_kernel(const float* __restrict__ t, int dim, OT* __restrict__ out) {
    const int b = blockIdx.x;
    const int half_dim = dim / 2;
    for (int k = threadIdx.x; k < half_dim; k += blockDim.x) {
        const float w = expf(-9.210340371976184f * (float)k / (float)half_dim);
        const float a = t[b] * w;
        out[(size_t)b * dim + k] = (OT)cosf(a);
        out[(size_t)b * dim + half_dim + k] = (OT)sinf(a);
    }
    if ((dim & 1) && threadIdx.x == 0) out[(size_t)b * dim + dim - 1] = (OT)0.0f;
}

// fp32 rows -> fp16 [hi | lo] rows (8 channels per thread)
__global__ void split_f32_kernel(const float* __restrict__ x, int ldx, size_t rows, int nvec, half_t* __restrict__ y, int ldy) {
    const size_t total = rows * (size_t)nvec;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)nvec;
        const int c = (int)(i - r * (size_t)nvec) * 8;
        const float4 a = *reinterpret_cast<const float4*>(x + r * ldx + c);
        const float4 b = *reinterpret_cast<const float4*>(x + r * ldx + c + 4);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        half8_t hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) { hi[j] = (half_t)v[j]; lo[j] = (half_t)(v[j] - (float)hi[j]); }
        st16(y + r * ldy + c, *reinterpret_cast<uint4*>(&hi));
        st16(y + r * ldy + (size_t)nvec * 8 + c, *reinterpret_cast<uint4*>(&lo));
    }
}

__global__ void silu_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, size_t nvec) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        uint4 raw = ld16(x + i * 8);
        const half8_t v = *reinterpret_cast<half8_t*>(&raw);
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)silu_f((float)v[j]);
        st16(y + i * 8, *reinterpret_cast<uint4*>(&o));
    }
}

// The operand scaffolding of the elementwise sampler kernels (latent_blend, ddim_update, dpmpp_update): VEC consecutive floats of one operand per
// thread, as one float4 (VEC = 4: 16-byte pointers) or one scalar.  Arrays by reference: they stay in registers.  No arithmetic here.
template <int VEC>
__device__ __forceinline__ void ew_load(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void ew_store(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// The sampler arithmetic follows the reference's operation order with contraction disabled so that,
// given identical eps, x_prev is bit-identical to torch fp32 (plms.py:123,126-161).  Every helper that holds a multiply-add is defined inside
// this region: above it, it would be contracted to FMA.
#pragma clang fp contract(off)
// classifier-free guidance on the [cond ; uncond] halves (reps == 2): e = e_u + g * (e_c - e_u); one half (reps == 1): e_c as it is, and eu
// (by reference: not loaded then) is not read
__device__ __forceinline__ float guided_eps(float ec, const float& eu, int reps, float guidance) {
    return reps == 2 ? eu + guidance * (ec - eu) : ec;
}

// three-branch guidance on the [cond ; text-only ; uncond] thirds: e = (e_u + s_t * (e_t - e_u)) + s_l * (e_c - e_t), left to right.  With
// s_l == s_t it is guided_eps up to rounding; with s_l == 0 the conditional third is weighted by zero
__device__ __forceinline__ float guided_eps3(float ec, float et, float eu, float s_text, float s_layout) {
    const float text = eu + s_text * (et - eu);
    return text + s_layout * (ec - et);
}

// The combine of a three-branch evaluation as one launch: eps3b fp32 [3n] -> e fp32 [n].  e aliases nothing.  VEC = 4: n % 4 == 0 and
// 16-byte pointers (then the thirds at eps3b + n and eps3b + 2n are 16-byte aligned too), one float4 per third per thread.
template <int VEC>
__global__ __launch_bounds__(256) void cfg3_combine_kernel(const float* __restrict__ eps3b, float s_text, float s_layout, size_t n,
                                                           float* __restrict__ e) {
    const size_t nvec = n / VEC;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i = v * VEC;
        float ec[VEC], et[VEC], eu[VEC], o[VEC];
        ew_load<VEC>(eps3b + i, ec);
        ew_load<VEC>(eps3b + n + i, et);
        ew_load<VEC>(eps3b + 2 * n + i, eu);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = guided_eps3(ec[j], et[j], eu[j], s_text, s_layout);
        ew_store<VEC>(e + i, o);
    }
}

__global__ void cfg_combine_kernel(const float* __restrict__ eps2b, float guidance, size_t n, float* __restrict__ e) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float ec = eps2b[i];
        const float eu = eps2b[n + i];
        e[i] = eu + guidance * (ec - eu);
    }
}

// No __restrict__: gl_plms_step updates in place (x == x_prev) and an eps term may alias the output; every access is
// same-index and element-wise, which is well defined only without the no-alias promise.
__global__ void plms_update_kernel(const float* x, const float* e, const float* e1, const float* e2, const float* e3, float c0, float c1,
                                   float c2, float c3, float div, float sqrt_at, float s1m, float sqrt_aprev,
                                   float dir_coef, size_t n, float* x_prev) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        // e' : (c0*e + c1*e1 + c2*e2 + c3*e3) / div, left to right as plms.py:146-159 writes it
        float ep = c0 * e[i];
        if (e1) ep = ep + c1 * e1[i];
        if (e2) ep = ep + c2 * e2[i];
        if (e3) ep = ep + c3 * e3[i];
        ep = ep / div;
        const float pred_x0 = (x[i] - s1m * ep) / sqrt_at;
        const float dir_xt = dir_coef * ep;
        x_prev[i] = sqrt_aprev * pred_x0 + dir_xt;
    }
}

// Masked PLMS step (plms.py:95-99 with ldm.py:19-22): x = (a * x0 + s * noise) * m + (1 - m) * x, in place, in torch's operation order
// (q_sample's two products and their sum, then img_orig * mask, (1 - mask) * img and the sum).  x0 / noise have batch 1 or B (nb0), the
// mask [1|B, 1, hw] (nbm).  VEC = 4: hw % 4 == 0, one float4 of one (b, c) row per thread.
template <int VEC>
__global__ __launch_bounds__(256) void latent_blend_kernel(float* x, const float* __restrict__ x0, const float* __restrict__ noise,
                                                           const float* __restrict__ m, float a, float s, int B, int C, int hw, int nb0,
                                                           int nbm) {
    const size_t nvec = (size_t)B * C * hw / VEC;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i = v * VEC;
        const int p = (int)(i % hw);
        const size_t bc = i / hw;
        const int c = (int)(bc % C), b = (int)(bc / C);
        const size_t i0 = ((size_t)(nb0 == 1 ? 0 : b) * C + c) * hw + p;
        const size_t im = (size_t)(nbm == 1 ? 0 : b) * hw + p;
        float xv[VEC], x0v[VEC], nv[VEC], mv[VEC];
        ew_load<VEC>(x + i, xv);
        ew_load<VEC>(x0 + i0, x0v);
        ew_load<VEC>(noise + i0, nv);
        ew_load<VEC>(m + im, mv);
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float q = a * x0v[j] + s * nv[j];
            o[j] = q * mv[j] + (1.0f - mv[j]) * xv[j];
        }
        ew_store<VEC>(x + i, o);
    }
}

// The forward process at one timestep (ldm.py:19-22, the blend's q_sample without the mask): out = a * x0 + s * noise on [B, chw], two
// products and their sum.  x0 has 1 or B (nb0) samples.  No __restrict__ on noise / out: out may be noise (in place on the running latent);
// every thread loads its operands before it stores.  VEC = 4: chw % 4 == 0, one float4 of one sample per thread.
template <int VEC>
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* noise, float a, float s, size_t chw, size_t n,
                                                       int nb0, float* out) {
    const size_t nvec = n / VEC;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i = v * VEC;
        float x0v[VEC], nv[VEC], o[VEC];
        ew_load<VEC>(x0 + (nb0 == 1 ? i % chw : i), x0v);
        ew_load<VEC>(noise + i, nv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = a * x0v[j] + s * nv[j];
        ew_store<VEC>(out + i, o);
    }
}

// One DDIM step behind the UNet (ddim.py:115-135) as ONE launch: the CFG combine of the [cond ; uncond] output (reps == 2), pred_x0 and
// x_prev, in the reference's operation order: e = e_u + g * (e_c - e_u); pred_x0 = (x - s1m * e) / sqrt_at;
// x_prev = (sqrt_aprev * pred_x0 + dir_coef * e) + sigma * noise.  noise == NULL (the reference's 0 * randn): the last term is SKIPPED, which
// gives the bits of adding the zero for every finite value.  No __restrict__ on x / x_out / pred_x0: the update runs in place; every thread
// reads all of its operands before it stores.  VEC = 4: n % 4 == 0 and 16-byte pointers, one float4 per operand per thread.
template <int VEC>
__global__ __launch_bounds__(256) void ddim_update_kernel(const float* eps, const float* x, const float* noise, int reps, float guidance,
                                                          float sqrt_at, float s1m, float sqrt_aprev, float dir_coef, float sigma, size_t n,
                                                          float* x_out, float* pred_out) {
    const size_t nvec = n / VEC;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i = v * VEC;
        float ec[VEC], eu[VEC], xv[VEC], nv[VEC];
        ew_load<VEC>(eps + i, ec);
        ew_load<VEC>(x + i, xv);
        if (reps == 2) ew_load<VEC>(eps + n + i, eu);
        if (noise) ew_load<VEC>(noise + i, nv);
        float o[VEC], p[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float e = guided_eps(ec[j], eu[j], reps, guidance);
            p[j] = (xv[j] - s1m * e) / sqrt_at;
            const float dir_xt = dir_coef * e;
            o[j] = sqrt_aprev * p[j] + dir_xt;
            if (noise) o[j] = o[j] + sigma * nv[j];
        }
        ew_store<VEC>(x_out + i, o);
        if (pred_out) ew_store<VEC>(pred_out + i, p);
    }
}

// One DPM-Solver++(2M) step behind the UNet (Lu et al., arXiv 2211.01095, Algorithm 2) as ONE launch: the CFG combine as above, then
// x0 = (x - s1m * e) / sqrt_at; D = w1 * x0 + w0 * x0_old; x_prev = c_x * x + c_d * D, left to right.  x0_old == NULL (a first-order step):
// D = w1 * x0.  No __restrict__ on x / x_out / x0_old / x0_out: x_out may be x and x0_out may be x0_old (ONE history buffer); every thread
// reads all of its operands before it stores, and no thread reads an element another thread writes.  VEC as for ddim_update_kernel.
template <int VEC>
__global__ __launch_bounds__(256) void dpmpp_update_kernel(const float* eps, const float* x, const float* x0_old, int reps, float guidance,
                                                           float sqrt_at, float s1m, float c_x, float c_d, float w1, float w0, size_t n,
                                                           float* x_out, float* x0_out) {
    const size_t nvec = n / VEC;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i = v * VEC;
        float ec[VEC], eu[VEC], xv[VEC], hv[VEC];
        ew_load<VEC>(eps + i, ec);
        ew_load<VEC>(x + i, xv);
        if (reps == 2) ew_load<VEC>(eps + n + i, eu);
        if (x0_old) ew_load<VEC>(x0_old + i, hv);
        float o[VEC], p[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float e = guided_eps(ec[j], eu[j], reps, guidance);
            p[j] = (xv[j] - s1m * e) / sqrt_at;
            float d = w1 * p[j];
            if (x0_old) d = d + w0 * hv[j];
            const float cx = c_x * xv[j];
            o[j] = cx + c_d * d;
        }
        ew_store<VEC>(x_out + i, o);
        ew_store<VEC>(x0_out + i, p);
    }
}
#pragma clang fp contract(fast)

// DiagonalGaussianDistribution(quant_conv(h)).sample() * scale_factor (autoencoder.py:34-38, distributions.py:24-36) per pixel:
// moments = W h + b (fp32 1x1 conv, 2E x Cin), mean / logvar = the two halves, logvar clamped to [-30, 20], std = exp(logvar / 2),
// z = (mean + std * noise) * scale.  h fp32 NCHW [B, Cin, hw]; z / mean fp32 NCHW [B, E, hw].  One thread per pixel.
__global__ __launch_bounds__(256) void vae_posterior_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ noise, float scale,
                                                            int B, int Cin, int E, int hw, float* __restrict__ z, float* __restrict__ mean) {
    const size_t n = (size_t)B * hw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw), p = (int)(i % hw);
        const float* hp = h + (size_t)b * Cin * hw + p;
        for (int e = 0; e < E; ++e) {
            float mu = bias[e], lv = bias[E + e];
            for (int k = 0; k < Cin; ++k) {
                const float hv = hp[(size_t)k * hw];
                mu += w[(size_t)e * Cin + k] * hv;
                lv += w[(size_t)(E + e) * Cin + k] * hv;
            }
            lv = fminf(fmaxf(lv, -30.0f), 20.0f);
            const float sd = expf(0.5f * lv);
            const size_t o = ((size_t)b * E + e) * hw + p;
            z[o] = (mu + sd * noise[o]) * scale;
            if (mean) mean[o] = mu;
        }
    }
}

// x fp32 [B, C, hw] -> fp16 [reps*B, hw, Cpad].  split: channels [0, C) = hi = fp16(x), [C, 2C) = lo = fp16(x - hi), [2C, 3C) = hi again -- against
// first-conv weights packed [Whi | Whi | Wlo] (weights.py pack_first_conv) the one conv launch computes xhi.Whi + xlo.Whi + xhi.Wlo in the channel
// padding it carries anyway (4 of 64 channels used)
__global__ void pack_latent_kernel(const float* __restrict__ x, int B, int C, int hw, int Cpad, int reps, int split,
                                   half_t* __restrict__ out) {
    const size_t total = (size_t)reps * B * hw * Cpad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const size_t t = i / Cpad;
        const int p = (int)(t % hw);
        const int rb = (int)(t / hw);
        const int b = rb % B;
        half_t o = (half_t)0.0f;
        if (c < C) {
            o = (half_t)x[((size_t)b * C + c) * hw + p];
        } else if (split && c < 3 * C) {
            const int cc = c < 2 * C ? c - C : c - 2 * C;
            const float v = x[((size_t)b * C + cc) * hw + p];
            const half_t hi = (half_t)v;
            o = c < 2 * C ? (half_t)(v - (float)hi) : hi;
        }
        out[i] = o;
    }
}

// pack_latent_kernel over the channel concatenation of two sources (an inpaint_mode UNet's first-conv input, openaimodel.py:439): x fp32 [B, C, hw]
// and extra fp32 [Bs, Ce, hw] (Bs = 1: one extra for every sample) -> fp16 [reps*B, hw, Cpad].  Ct = C + Ce: channels [0, Ct) = hi of [x | extra];
// split: [Ct, 2 Ct) = lo, [2 Ct, 3 Ct) = hi again; zero behind
__global__ void pack_latent_extra_kernel(const float* __restrict__ x, const float* __restrict__ extra, int B, int Bs, int C, int Ce, int hw,
                                         int Cpad, int reps, int split, half_t* __restrict__ out) {
    const int Ct = C + Ce, used = split ? 3 * Ct : Ct;
    const size_t total = (size_t)reps * B * hw * Cpad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const size_t t = i / Cpad;
        const int p = (int)(t % hw);
        const int rb = (int)(t / hw);
        const int b = rb % B;
        half_t o = (half_t)0.0f;
        if (c < used) {
            const int part = c / Ct, cc = c - part * Ct;
            const float v = cc < C ? x[((size_t)b * C + cc) * hw + p] : extra[((size_t)(Bs == 1 ? 0 : b) * Ce + (cc - C)) * hw + p];
            const half_t hi = (half_t)v;
            o = part == 1 ? (half_t)(v - (float)hi) : hi;
        }
        out[i] = o;
    }
}

// Row softmax in place over fp16 [rows, n] (row stride ld): the single-head d = C mid-block attention of
// the VAE decoder (model.py:180-186) runs as two GEMMs around this kernel because its head dim (512)
// exceeds the flash kernel's register budget; it runs once per image, not per step.
__global__ __launch_bounds__(256) void softmax_rows_kernel(half_t* __restrict__ x, int n, int ld, float scale) {
    __shared__ float red[4];
    half_t* row = x + (size_t)blockIdx.x * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mx = -INFINITY;
    for (int i = threadIdx.x * 8; i < n; i += 256 * 8) {
        uint4 raw = ld16(row + i);
        const half8_t v = *reinterpret_cast<half8_t*>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, (float)v[j]);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * scale;
    __syncthreads();
    float sum = 0.0f;
    for (int i = threadIdx.x * 8; i < n; i += 256 * 8) {
        uint4 raw = ld16(row + i);
        const half8_t v = *reinterpret_cast<half8_t*>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += __expf((float)v[j] * scale - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
    for (int i = threadIdx.x * 8; i < n; i += 256 * 8) {
        uint4 raw = ld16(row + i);
        const half8_t v = *reinterpret_cast<half8_t*>(&raw);
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)(__expf((float)v[j] * scale - mx) * inv);
        st16(row + i, *reinterpret_cast<uint4*>(&o));
    }
}

// z fp32 [B, C, hw] -> fp16 [B, hw, Cpad]: out[:, :, co] = bias[co] + sum_ci w[co, ci] * (z[:, ci, :] * pre),
// zero for co >= C.  AutoencoderKL.decode's 1/scale_factor and 1x1 post_quant_conv (autoencoder.py:41-42).
__global__ void latent_affine_pack_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                          const float* __restrict__ bias, float pre, int B, int C, int hw, int Cpad,
                                          half_t* __restrict__ out) {
    const size_t total = (size_t)B * hw * Cpad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cpad);
        const size_t t = i / Cpad;
        const int p = (int)(t % hw);
        const int b = (int)(t / hw);
        float v = 0.0f;
        if (co < C) {
            v = bias[co];
            for (int ci = 0; ci < C; ++ci) v += w[co * C + ci] * (z[((size_t)b * C + ci) * hw + p] * pre);
        }
        out[i] = (half_t)v;
    }
}

int ew_blocks(size_t n) {
    size_t b = (n + 255) / 256;
    return (int)(b > 2048 ? 2048 : (b == 0 ? 1 : b));
}

// The float4 form (<4>) of an elementwise sampler kernel, else the scalar one (<1>): ``n`` -- the element count, or the row length a vector
// must not cross -- is a multiple of 4 and every non-null operand is 16-byte aligned.
bool ew_vec4(size_t n, std::initializer_list<const void*> operands) {
    uintptr_t bits = 0;
    for (const void* p : operands) bits |= reinterpret_cast<uintptr_t>(p);
    return (n % 4) == 0 && (bits % 16) == 0;
}

}  // namespace

extern "C" int gl_posnet_input(const float* boxes, const float* masks, const float* emb, const float* null_pos,
                               const float* null_xyxy, int32_t rows, int32_t in_dim, int32_t num_freqs, void* out,
                               void* stream) {
    if (!boxes || !masks || !emb || !null_pos || !null_xyxy || !out || rows <= 0) return GL_ERR_BAD_ARG;
    posnet_input_kernel<half_t><<<dim3(rows), dim3(256), 0, (hipStream_t)stream>>>(boxes, masks, emb, null_pos, null_xyxy, in_dim,
                                                                                   num_freqs, reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_posnet_input_f32(const float* boxes, const float* masks, const float* emb, const float* null_pos,
                                   const float* null_xyxy, int32_t rows, int32_t in_dim, int32_t num_freqs, float* out, void* stream) {
    if (!boxes || !masks || !emb || !null_pos || !null_xyxy || !out || rows <= 0) return GL_ERR_BAD_ARG;
    posnet_input_kernel<float><<<dim3(rows), dim3(256), 0, (hipStream_t)stream>>>(boxes, masks, emb, null_pos, null_xyxy, in_dim, num_freqs, out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_posnet_input_ti(const float* boxes, const float* masks, const float* text_masks, const float* image_masks, const float* text_emb,
                                  const float* image_emb, const float* null_text, const float* null_image, const float* null_xyxy, int32_t rows,
                                  int32_t in_dim, int32_t num_freqs, void* out_text, void* out_image, void* stream) {
    if (!boxes || !masks || !text_masks || !image_masks || !text_emb || !image_emb || !null_text || !null_image || !null_xyxy || !out_text ||
        !out_image || rows <= 0 || in_dim <= 0 || num_freqs <= 0)
        return GL_ERR_BAD_ARG;
    posnet_input_ti_kernel<half_t><<<dim3(rows), dim3(256), 0, (hipStream_t)stream>>>(boxes, masks, text_masks, image_masks, text_emb, image_emb, null_text,
                                                                                      null_image, null_xyxy, in_dim, num_freqs,
                                                                                      reinterpret_cast<half_t*>(out_text), reinterpret_cast<half_t*>(out_image));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_posnet_input_ti_f32(const float* boxes, const float* masks, const float* text_masks, const float* image_masks,
                                      const float* text_emb, const float* image_emb, const float* null_text, const float* null_image,
                                      const float* null_xyxy, int32_t rows, int32_t in_dim, int32_t num_freqs, float* out_text, float* out_image,
                                      void* stream) {
    if (!boxes || !masks || !text_masks || !image_masks || !text_emb || !image_emb || !null_text || !null_image || !null_xyxy || !out_text ||
        !out_image || rows <= 0 || in_dim <= 0 || num_freqs <= 0)
        return GL_ERR_BAD_ARG;
    posnet_input_ti_kernel<float><<<dim3(rows), dim3(256), 0, (hipStream_t)stream>>>(boxes, masks, text_masks, image_masks, text_emb, image_emb, null_text,
                                                                                     null_image, null_xyxy, in_dim, num_freqs, out_text, out_image);
    GL_CHECK_LAUNCH();
    return 0;
}

template <typename OT>
static int posnet_input_kp(const float* points, const float* masks, const float* person_emb, const float* keypoint_emb, const float* null_person,
                           const float* null_xy, int32_t B, int32_t tokens, int32_t D, int32_t num_freqs, OT* out, void* stream) {
    if (!points || !masks || !person_emb || !keypoint_emb || !null_person || !null_xy || !out || B <= 0 || tokens <= 0 || (tokens % 17) != 0 || D <= 0 ||
        num_freqs <= 0)
        return GL_ERR_BAD_ARG;
    const int ld = (D + 4 * num_freqs + 63) / 64 * 64;
    posnet_input_kp_kernel<OT><<<dim3(B * tokens), dim3(256), 0, (hipStream_t)stream>>>(points, masks, person_emb, keypoint_emb, null_person, null_xy,
                                                                                       tokens, D, num_freqs, ld, out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_posnet_input_kp(const float* points, const float* masks, const float* person_emb, const float* keypoint_emb,
                                  const float* null_person, const float* null_xy, int32_t B, int32_t tokens, int32_t D, int32_t num_freqs, void* out,
                                  void* stream) {
    return posnet_input_kp(points, masks, person_emb, keypoint_emb, null_person, null_xy, B, tokens, D, num_freqs, reinterpret_cast<half_t*>(out), stream);
}

extern "C" int gl_posnet_input_kp_f32(const float* points, const float* masks, const float* person_emb, const float* keypoint_emb,
                                      const float* null_person, const float* null_xy, int32_t B, int32_t tokens, int32_t D, int32_t num_freqs,
                                      float* out, void* stream) {
    return posnet_input_kp(points, masks, person_emb, keypoint_emb, null_person, null_xy, B, tokens, D, num_freqs, out, stream);
}

extern "C" int gl_image_ground_feature(const float* feat, const float* proj, int32_t n, int32_t dim, float norm, float* out, void* stream) {
    if (!feat || !proj || !out || n <= 0 || dim <= 0 || dim > 1024) return GL_ERR_BAD_ARG;
    image_ground_feature_kernel<<<dim3(n), dim3(256), 0, (hipStream_t)stream>>>(feat, proj, dim, norm, out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_timestep_embedding_f32(const float* t, int32_t B, int32_t dim, float* out, void* stream) {
    if (!t || !out || B <= 0 || dim <= 0) return GL_ERR_BAD_ARG;
    timestep_embedding_kernel<float><<<dim3(B), dim3(256), 0, (hipStream_t)stream>>>(t, dim, out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_split_f32(const float* x, int32_t ldx, int64_t rows, int32_t C, void* y, int32_t ldy, void* stream) {
    if (!x || !y || rows <= 0 || C <= 0 || (C % 8) || (ldx % 4) || (ldy % 8) || ldy < 2 * C || ldx < C) return GL_ERR_BAD_ARG;
    const size_t total = (size_t)rows * (C / 8);
    split_f32_kernel<<<dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream>>>(x, ldx, (size_t)rows, C / 8, reinterpret_cast<half_t*>(y), ldy);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_timestep_embedding(const float* t, int32_t B, int32_t dim, void* out, void* stream) {
    if (!t || !out || B <= 0 || dim <= 0) return GL_ERR_BAD_ARG;
    timestep_embedding_kernel<half_t><<<dim3(B), dim3(256), 0, (hipStream_t)stream>>>(t, dim, reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_silu_f16(const void* x, void* y, int64_t n, void* stream) {
    if (!x || !y || n <= 0 || (n % 8)) return GL_ERR_BAD_ARG;
    silu_kernel<<<dim3(ew_blocks((size_t)n / 8)), dim3(256), 0, (hipStream_t)stream>>>(
        reinterpret_cast<const half_t*>(x), reinterpret_cast<half_t*>(y), (size_t)n / 8);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_cfg_combine(const float* eps2b, float guidance, int64_t n, float* e_out, void* stream) {
    if (!eps2b || !e_out || n <= 0) return GL_ERR_BAD_ARG;
    cfg_combine_kernel<<<dim3(ew_blocks((size_t)n)), dim3(256), 0, (hipStream_t)stream>>>(eps2b, guidance, (size_t)n, e_out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_cfg3_combine(const float* eps3b, float s_text, float s_layout, int64_t n, float* e_out, void* stream) {
    if (!eps3b || !e_out || n <= 0) return GL_ERR_BAD_ARG;
    if (ew_vec4((size_t)n, {eps3b, e_out}))
        cfg3_combine_kernel<4><<<dim3(ew_blocks((size_t)n / 4)), dim3(256), 0, (hipStream_t)stream>>>(eps3b, s_text, s_layout, (size_t)n, e_out);
    else
        cfg3_combine_kernel<1><<<dim3(ew_blocks((size_t)n)), dim3(256), 0, (hipStream_t)stream>>>(eps3b, s_text, s_layout, (size_t)n, e_out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_plms_update(const float* x, const float* e, const float* e1, const float* e2, const float* e3, float c0,
                              float c1, float c2, float c3, float div, float sqrt_at, float s1m, float sqrt_aprev,
                              float dir_coef, int64_t n, float* x_prev, void* stream) {
    if (!x || !e || !x_prev || n <= 0) return GL_ERR_BAD_ARG;
    plms_update_kernel<<<dim3(ew_blocks((size_t)n)), dim3(256), 0, (hipStream_t)stream>>>(
        x, e, e1, e2, e3, c0, c1, c2, c3, div, sqrt_at, s1m, sqrt_aprev, dir_coef, (size_t)n, x_prev);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_ddim_update(const float* eps, const float* x, const float* noise, int32_t reps, float guidance, float sqrt_at, float s1m,
                              float sqrt_aprev, float dir_coef, float sigma, int64_t n, float* x_out, float* pred_x0, void* stream) {
    if (!eps || !x || !x_out || n <= 0 || (reps != 1 && reps != 2)) return GL_ERR_BAD_ARG;
    if (ew_vec4((size_t)n, {eps, x, noise, x_out, pred_x0}))
        ddim_update_kernel<4><<<dim3(ew_blocks((size_t)n / 4)), dim3(256), 0, (hipStream_t)stream>>>(
            eps, x, noise, reps, guidance, sqrt_at, s1m, sqrt_aprev, dir_coef, sigma, (size_t)n, x_out, pred_x0);
    else
        ddim_update_kernel<1><<<dim3(ew_blocks((size_t)n)), dim3(256), 0, (hipStream_t)stream>>>(
            eps, x, noise, reps, guidance, sqrt_at, s1m, sqrt_aprev, dir_coef, sigma, (size_t)n, x_out, pred_x0);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_dpmpp_update(const float* eps, const float* x, const float* x0_old, int32_t reps, float guidance, float sqrt_at, float s1m,
                               float c_x, float c_d, float w1, float w0, int64_t n, float* x_out, float* x0_out, void* stream) {
    if (!eps || !x || !x_out || !x0_out || n <= 0 || (reps != 1 && reps != 2)) return GL_ERR_BAD_ARG;
    if (!x0_old && w0 != 0.0f) return GL_ERR_BAD_ARG;       // a first-order step has no history term
    if (ew_vec4((size_t)n, {eps, x, x0_old, x_out, x0_out}))
        dpmpp_update_kernel<4><<<dim3(ew_blocks((size_t)n / 4)), dim3(256), 0, (hipStream_t)stream>>>(
            eps, x, x0_old, reps, guidance, sqrt_at, s1m, c_x, c_d, w1, w0, (size_t)n, x_out, x0_out);
    else
        dpmpp_update_kernel<1><<<dim3(ew_blocks((size_t)n)), dim3(256), 0, (hipStream_t)stream>>>(
            eps, x, x0_old, reps, guidance, sqrt_at, s1m, c_x, c_d, w1, w0, (size_t)n, x_out, x0_out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_pack_latent(const float* x, int32_t B, int32_t C, int32_t hw, int32_t Cpad, int32_t reps, int32_t split, void* out,
                              void* stream) {
    if (!x || !out || B <= 0 || C <= 0 || hw <= 0 || Cpad < (split ? 3 * C : C) || reps <= 0) return GL_ERR_BAD_ARG;
    pack_latent_kernel<<<dim3(ew_blocks((size_t)reps * B * hw * Cpad)), dim3(256), 0, (hipStream_t)stream>>>(
        x, B, C, hw, Cpad, reps, split, reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_pack_latent_extra(const float* x, const float* extra, int32_t B, int32_t Bs, int32_t C, int32_t Ce, int32_t hw, int32_t Cpad,
                                    int32_t reps, int32_t split, void* out, void* stream) {
    if (!x || !extra || !out || B <= 0 || C <= 0 || Ce <= 0 || hw <= 0 || reps <= 0 || (Bs != 1 && Bs != B)) return GL_ERR_BAD_ARG;
    if (Cpad < (split ? 3 : 1) * (C + Ce)) return GL_ERR_BAD_ARG;
    pack_latent_extra_kernel<<<dim3(ew_blocks((size_t)reps * B * hw * Cpad)), dim3(256), 0, (hipStream_t)stream>>>(
        x, extra, B, Bs, C, Ce, hw, Cpad, reps, split, reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_latent_blend(float* x, const float* x0, const float* noise, const float* mask, float a, float s, int32_t B, int32_t C,
                               int32_t hw, int32_t x0_batch, int32_t mask_batch, void* stream) {
    if (!x || !x0 || !noise || !mask || B <= 0 || C <= 0 || hw <= 0) return GL_ERR_BAD_ARG;
    if ((x0_batch != 1 && x0_batch != B) || (mask_batch != 1 && mask_batch != B)) return GL_ERR_BAD_ARG;
    const size_t n = (size_t)B * C * hw;
    if (ew_vec4((size_t)hw, {x, x0, noise, mask}))       // a float4 stays inside one (b, c) row
        latent_blend_kernel<4><<<dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream>>>(x, x0, noise, mask, a, s, B, C, hw, x0_batch, mask_batch);
    else
        latent_blend_kernel<1><<<dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream>>>(x, x0, noise, mask, a, s, B, C, hw, x0_batch, mask_batch);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_q_sample(const float* x0, const float* noise, float a, float s, int32_t B, int32_t chw, int32_t x0_batch, float* out,
                           void* stream) {
    if (!x0 || !noise || !out || B <= 0 || chw <= 0 || (x0_batch != 1 && x0_batch != B)) return GL_ERR_BAD_ARG;
    const size_t n = (size_t)B * chw;
    if (ew_vec4((size_t)chw, {x0, noise, out}))          // a float4 stays inside one sample
        q_sample_kernel<4><<<dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream>>>(x0, noise, a, s, (size_t)chw, n, x0_batch, out);
    else
        q_sample_kernel<1><<<dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream>>>(x0, noise, a, s, (size_t)chw, n, x0_batch, out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_vae_posterior(const float* h, const float* w, const float* bias, const float* noise, float scale, int32_t B, int32_t Cin,
                                int32_t E, int32_t hw, float* z, float* mean, void* stream) {
    if (!h || !w || !bias || !noise || !z || B <= 0 || Cin <= 0 || E <= 0 || hw <= 0) return GL_ERR_BAD_ARG;
    vae_posterior_kernel<<<dim3(ew_blocks((size_t)B * hw)), dim3(256), 0, (hipStream_t)stream>>>(h, w, bias, noise, scale, B, Cin, E, hw, z, mean);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_softmax_rows(void* x, int32_t rows, int32_t n, int32_t ld, float scale, void* stream) {
    if (!x || rows <= 0 || n <= 0 || (n % 8) || (ld % 8)) return GL_ERR_BAD_ARG;
    softmax_rows_kernel<<<dim3(rows), dim3(256), 0, (hipStream_t)stream>>>(reinterpret_cast<half_t*>(x), n, ld, scale);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_latent_affine_pack(const float* z, const float* w, const float* bias, float pre, int32_t B, int32_t C,
                                     int32_t hw, int32_t Cpad, void* out, void* stream) {
    if (!z || !w || !bias || !out || B <= 0 || C <= 0 || hw <= 0 || Cpad < C) return GL_ERR_BAD_ARG;
    latent_affine_pack_kernel<<<dim3(ew_blocks((size_t)B * hw * Cpad)), dim3(256), 0, (hipStream_t)stream>>>(
        z, w, bias, pre, B, C, hw, Cpad, reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_init_gemm(void);
extern "C" int gl_init_ff(void);
extern "C" int gl_init_attn(void);
// ---- option table (opts.h): process defaults, per-thread effective table of the running handle
static gl_opts make_default_opts() {
    gl_opts o{};
    o.v[2] = 0;    o.v[3] = 0;    o.v[4] = 400;  o.v[5] = 300;  o.v[GL_OPT_SPLITK_TILES_CONV] = 450;
    o.v[6] = 16;   o.v[7] = 300;  o.v[8] = 1;    o.v[10] = -1;  o.v[13] = 3;
    o.v[16] = 16;  o.v[17] = 1;   o.v[20] = 0;   o.v[21] = 1;   o.v[23] = 1;
    o.v[24] = 64;  o.v[25] = 1;   o.v[27] = 1;   o.v[29] = 1;   o.v[30] = 1;
    o.v[31] = 200; o.v[32] = 0;   o.v[33] = 0;   o.v[34] = 11;  o.v[35] = 5;
    o.v[37] = 1;
    o.v[41] = 1;
    o.v[42] = 1;
    o.v[43] = 1;
    o.v[38] = 1;
    o.v[44] = 1;
    o.v[45] = 1024;
    o.v[46] = 11;
    o.v[47] = 100;
    o.v[50] = 0;       // strict mode (handles created with split_weights)
    o.v[51] = 1;       // ... with the third pass x.Wlo
    o.v[52] = 1;       // three-pass products on the dedicated three-pass loop of the 8-wave kernel (gemm8.hip S3; 0 = K-walk)
    o.v[55] = 2;       // upsample convs as four folded 2x2 convs (gemm8.hip UPF), read when a handle is CREATED (it decides the weight table): 0 / 2 = a handle
                       // keeps [Cout, 9 Cin] rows, 1 = folded [4 Cout, 4 Cin]; 2 (default) tells the Python packers to fold by their measured rule
    o.v[54] = 2;       // kx-reuse loop of the 8-wave 3x3 conv (gemm8.hip KXR): 0 never, 1 wherever eligible, 2 = the measured shapes
    return o;
}
gl_opts g_gl_opts = make_default_opts();
thread_local const gl_opts* tl_gl_opts = nullptr;
int g_gl_option_epoch = 0;

bool gl_opts_put(gl_opts& t, int key, int value) {
    switch (key) {
        case 2: case 3: case 4: case 6: case 7: case 8: case 10: case 13: case 17: case 20: case 21: case 23: case 24: case 25:
        case 27: case 29: case 30: case 31: case 32: case 33: case 35: case 37: case 38: case 41: case 42: case 43: case 44: case 45: case 46: case 47: case 50: case 51: case 52: case 53: case 54: case 55:
            t.v[key] = value;
            return true;
        case 5:                                  // < 0: the built-in thresholds (plain GEMM 300 tiles, conv 450)
            t.v[5] = value < 0 ? 300 : value;
            t.v[GL_OPT_SPLITK_TILES_CONV] = value < 0 ? 450 : value;
            return true;
        case 16: t.v[16] = value > 0 ? value : 16; return true;
        case 34: t.v[34] = value < 1 ? 1 : value; return true;
        default: return false;
    }
}

extern "C" int gl_get_option(int key) {
    if (key < 0 || key >= GL_OPT_MAX) return GL_ERR_BAD_ARG;
    return g_gl_opts.v[key];
}

extern "C" int gl_set_option(int key, int value) {
    if (key < 0 || key >= GL_OPT_MAX || !gl_opts_put(g_gl_opts, key, value)) return GL_ERR_BAD_ARG;
    ++g_gl_option_epoch;
    return 0;
}

extern "C" int gl_abi_version(void) { return GL_ABI_VERSION; }
extern "C" int gl_sizeof_gemm_args(void) { return (int)sizeof(gl_gemm_args); }
extern "C" int gl_sizeof_conv_args(void) { return (int)sizeof(gl_conv_args); }
extern "C" int gl_sizeof_attn_args(void) { return (int)sizeof(gl_attn_args); }
extern "C" int gl_sizeof_gn_args(void) { return (int)sizeof(gl_gn_args); }
extern "C" int gl_init(void) {
    int e = gl_init_gemm();
    if (!e) e = gl_init_ff();
    return e ? e : gl_init_attn();
}
