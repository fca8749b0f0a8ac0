// Kernels of the spatial grounding families (GLIGEN's canny / hed / depth / normal checkpoints): the ConvNeXt tokenizer of
// {canny,hed,depth,normal}_grounding_net.PositionNet (convnext.py) and the *_grounding_downsampler.  Both run ONCE per image, never per step;
// the matrix work of the tokenizer (stem / pointwise / downsample convs, the three linears) runs on gl_gemm, what is here are the stages around it:
//   gl_sp_stem_patchify   nearest resize (F.interpolate default) + 4x4 stride-4 patch rows of the stem conv, fp16 [B * (R/4)^2, 64]
//   gl_sp_layernorm       LayerNorm over the channels of fp32 rows, fp32 out (the stem's channels-first norm on NHWC rows)
//   gl_sp_dwconv_ln       depthwise 7x7 (pad 3) + LayerNorm over C, fp32 NHWC stream -> fp16 rows of pwconv1 (row stride padded to 64, pad zeroed)
//   gl_sp_gelu            erf-GELU on fp16 rows (between pwconv1 and pwconv2)
//   gl_sp_down_gather     per-pixel LayerNorm + gather of each 2x2 patch into one fp16 row [.., 4 C] (the 2x2 stride-2 conv as a GEMM operand)
//   gl_sp_assemble        feat * mask + null * (1 - mask) + pos -> fp16 rows of linears.0
//   gl_sp_bicubic         torch-semantics bicubic resize from host-built index / weight tables, fp32
//   gl_sp_conv4x4s2       direct 4x4 stride-2 pad-1 conv with an optional SiLU, fp32 FMA (1-8 channels: no matrix cores)
// Everything is bandwidth- or latency-bound and small; plain HIP C++, vector stores only.
#include "common.h"
#include "gligen_hip.h"

namespace {

constexpr float SP_EPS = 1e-6f;       // every LayerNorm of convnext.py

// F.interpolate(mode="nearest"): src = min(floor(dst * (float)in / out), in - 1), the scale in fp32 as torch computes it
__device__ __forceinline__ int nearest_src(int dst, int in, int out) {
    const int s = (int)floorf((float)dst * ((float)in / (float)out));
    return s < in - 1 ? s : in - 1;
}

// one block per patch row (b, py, px) of the R x R resized map; K index = (c * 4 + i) * 4 + j (the stem weight [C0, 3, 4, 4] flattened), 48 -> 64
__global__ __launch_bounds__(64) void stem_patchify_kernel(const float* __restrict__ map, int S, int R, half_t* __restrict__ out) {
    const int np = R / 4;
    const int row = blockIdx.x;
    const int b = row / (np * np), pi = row - b * np * np;
    const int py = pi / np, px = pi - py * np;
    const int k = threadIdx.x;
    float v = 0.0f;
    if (k < 48) {
        const int c = k >> 4, i = (k >> 2) & 3, j = k & 3;
        const int sy = nearest_src(py * 4 + i, S, R), sx = nearest_src(px * 4 + j, S, R);
        v = map[(((size_t)b * 3 + c) * S + sy) * S + sx];
    }
    out[(size_t)row * 64 + k] = (half_t)v;
}

// one wave per row, 4 rows per block: two passes over the row (mean, then centred variance), fp32
template <typename OT>
__device__ __forceinline__ void ln_row(const float* __restrict__ x, int C, const float* __restrict__ g, const float* __restrict__ b, OT* __restrict__ y,
                                       int lane) {
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s += x[c];
    const float mean = wave_sum(s) / (float)C;
    float q = 0.0f;
    for (int c = lane; c < C; c += 64) { const float d = x[c] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + SP_EPS);
    for (int c = lane; c < C; c += 64) y[c] = (OT)((x[c] - mean) * rstd * g[c] + b[c]);
}

__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* __restrict__ x, int64_t rows, int C, const float* __restrict__ g,
                                                             const float* __restrict__ b, float* __restrict__ y) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    ln_row(x + row * C, C, g, b, y + row * C, threadIdx.x & 63);
}

// Depthwise 7x7 + LayerNorm.  One block = DW_TW output pixels of one image row, all C channels, 256 threads.
// Channels go through LDS in chunks of DW_CC = 64: the chunk's 49 x 64 weights (12 544 B) and its 7-row x (DW_TW + 6)-column input window
// (7 * 14 * 64 * 4 = 25 088 B, zero outside the map) are staged, then thread (cl = t & 63, pg = t >> 6) accumulates channel cl of output pixels
// 2 pg and 2 pg + 1: consecutive lanes read consecutive channels (no bank conflicts), the two pixels share every weight read.  The conv rows
// (+ bias) stay in LDS as fp32 [DW_TW][C] (3 072 B at C = 96 .. 24 576 B at C = 768) until every chunk is done; then wave w normalises pixels
// 2 w and 2 w + 1 over C and writes fp16 rows of ldo columns, the pad columns [C, ldo) as zeros.
// LDS per block = 37 632 + 32 C bytes: 40 704 (C = 96), 43 776 (192), 49 920 (384), 62 208 (768) -> 3 blocks (12 waves) per CU of 160 KiB up to
// C = 384, 2 blocks (8 waves) at C = 768, where the map is 8 x 8 and the grid has 8 B blocks anyway.
constexpr int DW_TW = 8, DW_CC = 64, DW_WIN = DW_TW + 6;
__global__ __launch_bounds__(256) void dwconv_ln_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                        const float* __restrict__ g, const float* __restrict__ beta, int H, int W, int C, int ldo,
                                                        half_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* wl = sm;                                  // [49][DW_CC]
    float* win = wl + 49 * DW_CC;                    // [7][DW_WIN][DW_CC]
    float* rowbuf = win + 7 * DW_WIN * DW_CC;        // [DW_TW][C]
    const int xt = (W + DW_TW - 1) / DW_TW;
    int bid = blockIdx.x;
    const int tx = bid % xt; bid /= xt;
    const int y = bid % H;
    const int b = bid / H;
    const int x0 = tx * DW_TW;
    const int t = threadIdx.x, cl = t & 63, pg = t >> 6;
    for (int c0 = 0; c0 < C; c0 += DW_CC) {
        const bool cin = c0 + cl < C;
        __syncthreads();                             // the previous chunk's readers are done
        for (int i = pg; i < 49; i += 4) wl[i * DW_CC + cl] = cin ? w[(size_t)i * C + c0 + cl] : 0.0f;
        for (int i = pg; i < 7 * DW_WIN; i += 4) {
            const int r = i / DW_WIN, col = i - r * DW_WIN;
            const int sy = y + r - 3, sx = x0 + col - 3;
            float v = 0.0f;
            if (cin && sy >= 0 && sy < H && sx >= 0 && sx < W) v = x[(((size_t)b * H + sy) * W + sx) * C + c0 + cl];
            win[i * DW_CC + cl] = v;
        }
        __syncthreads();
        float a0 = 0.0f, a1 = 0.0f;
        const int p0 = 2 * pg;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            float col[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) col[k] = win[(ky * DW_WIN + p0 + k) * DW_CC + cl];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float wv = wl[(ky * 7 + kx) * DW_CC + cl];
                a0 = fmaf(wv, col[kx], a0);
                a1 = fmaf(wv, col[kx + 1], a1);
            }
        }
        if (cin) {
            const float bv = bias[c0 + cl];
            rowbuf[p0 * C + c0 + cl] = a0 + bv;
            rowbuf[(p0 + 1) * C + c0 + cl] = a1 + bv;
        }
    }
    __syncthreads();
    for (int p = 2 * pg; p < 2 * pg + 2; ++p) {
        if (x0 + p >= W) continue;                   // (uniform per wave)
        half_t* o = out + (((size_t)b * H + y) * W + x0 + p) * ldo;
        ln_row(rowbuf + p * C, C, g, beta, o, cl);
        for (int c = C + cl; c < ldo; c += 64) o[c] = (half_t)0.0f;
    }
}

// erf-GELU (nn.GELU default) on fp16 values, fp32 arithmetic.  0.5 x (1 + erf(x / sqrt 2)) = 0.5 x erfc(-x / sqrt 2): the erfc form keeps
// its relative accuracy in the negative tail, where 1 + erf cancels
__global__ __launch_bounds__(256) void gelu_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i >= n) return;                              // n is even
    const half2_t v = *reinterpret_cast<const half2_t*>(x + i);
    half2_t r;
    const float a = (float)v[0], c = (float)v[1];
    r[0] = (half_t)(0.5f * a * erfcf(-a * 0.70710678118654752440f));
    r[1] = (half_t)(0.5f * c * erfcf(-c * 0.70710678118654752440f));
    *reinterpret_cast<half2_t*>(y + i) = r;
}

// one wave per INPUT pixel (b, y, x): LayerNorm over C, written to output row (b, y / 2, x / 2) at columns [((y & 1) * 2 + (x & 1)) * C, + C)
// (the packed 2x2 weight is [Cout, ky, kx, Cin])
__global__ __launch_bounds__(256) void down_gather_kernel(const float* __restrict__ x, int B, int H, int W, int C, const float* __restrict__ g,
                                                          const float* __restrict__ b, half_t* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (int64_t)B * H * W) return;
    const int px = (int)(pix % W);
    const int py = (int)((pix / W) % H);
    const int bi = (int)(pix / ((int64_t)W * H));
    const int64_t orow = ((int64_t)bi * (H / 2) + (py >> 1)) * (W / 2) + (px >> 1);
    ln_row(x + pix * C, C, g, b, out + orow * 4 * C + ((py & 1) * 2 + (px & 1)) * C, threadIdx.x & 63);
}

// row (b, t): feat * m + null * (1 - m) + pos[t], m = mask[b] (a blend factor, as the reference computes it)
__global__ __launch_bounds__(256) void assemble_kernel(const float* __restrict__ feat, const float* __restrict__ mask, const float* __restrict__ null_f,
                                                       const float* __restrict__ pos, int T, int C, half_t* __restrict__ out) {
    const int row = blockIdx.x;
    const int b = row / T, t = row - b * T;
    const float m = mask[b];
    for (int c = threadIdx.x; c < C; c += 256) {
        const float o = feat[(size_t)row * C + c] * m + null_f[c] * (1.0f - m);
        out[(size_t)row * C + c] = (half_t)(o + pos[(size_t)t * C + c]);
    }
}

// out[b, c, oy, ox] = sum_i wy[oy][i] * (sum_j wx[ox][j] * in[b, c, iy[oy][i], ix[ox][j]]), c in [0, C) of the input's Ct channels.
// The tables (spatial.bicubic_table) hold torch's clamped source indices and its A = -0.75 coefficients, so any in / out size is one kernel.
__global__ __launch_bounds__(256) void bicubic_kernel(const float* __restrict__ in, int Ct, int C, int Hin, int Win, const int* __restrict__ iy,
                                                      const float* __restrict__ wy, const int* __restrict__ ix, const float* __restrict__ wx, int Hout,
                                                      int Wout, int64_t total, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % Wout);
    const int oy = (int)((idx / Wout) % Hout);
    const int c = (int)((idx / ((int64_t)Wout * Hout)) % C);
    const int b = (int)(idx / ((int64_t)Wout * Hout * C));
    const float* p = in + ((size_t)b * Ct + c) * Hin * Win;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* r = p + (size_t)iy[oy * 4 + i] * Win;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(wx[ox * 4 + j], r[ix[ox * 4 + j]], s);
        acc = fmaf(wy[oy * 4 + i], s, acc);
    }
    out[idx] = acc;
}

// Conv2d(Ci, Co, 4, 2, 1) on fp32 NCHW, one thread per output value; Ci, Co <= 8
__global__ __launch_bounds__(256) void conv4x4s2_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, int Ci,
                                                        int Co, int Hin, int Win, int silu, int64_t total, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int Ho = Hin / 2, Wo = Win / 2;
    const int ox = (int)(idx % Wo);
    const int oy = (int)((idx / Wo) % Ho);
    const int co = (int)((idx / ((int64_t)Wo * Ho)) % Co);
    const int b = (int)(idx / ((int64_t)Wo * Ho * Co));
    float acc = bias[co];
    for (int ci = 0; ci < Ci; ++ci) {
        const float* p = in + ((size_t)b * Ci + ci) * Hin * Win;
        const float* wk = w + ((size_t)co * Ci + ci) * 16;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const int sy = 2 * oy - 1 + ky;
            if (sy < 0 || sy >= Hin) continue;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const int sx = 2 * ox - 1 + kx;
                if (sx < 0 || sx >= Win) continue;
                acc = fmaf(wk[ky * 4 + kx], p[(size_t)sy * Win + sx], acc);
            }
        }
    }
    out[idx] = silu ? acc / (1.0f + expf(-acc)) : acc;
}

}  // namespace

extern "C" int gl_sp_stem_patchify(const float* map, int32_t B, int32_t S, int32_t R, void* out, void* stream) {
    if (!map || !out || B <= 0 || S <= 0 || R <= 0 || (R % 4) != 0) return GL_ERR_BAD_ARG;
    stem_patchify_kernel<<<dim3(B * (R / 4) * (R / 4)), dim3(64), 0, (hipStream_t)stream>>>(map, S, R, reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sp_layernorm(const float* x, int64_t rows, int32_t C, const float* gamma, const float* beta, float* y, void* stream) {
    if (!x || !gamma || !beta || !y || rows <= 0 || C <= 0 || rows > (int64_t)4 * 0x7fffffff) return GL_ERR_BAD_ARG;
    layernorm_rows_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(x, rows, C, gamma, beta, y);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sp_dwconv_ln(const float* x, const float* w, const float* bias, const float* ln_gamma, const float* ln_beta, int32_t B, int32_t H,
                               int32_t W, int32_t C, int32_t ldo, void* out, void* stream) {
    if (!x || !w || !bias || !ln_gamma || !ln_beta || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 768 || ldo < C || (ldo % 64) != 0)
        return GL_ERR_BAD_ARG;
    const int64_t blocks = (int64_t)B * H * ((W + DW_TW - 1) / DW_TW);
    if (blocks > 0x7fffffff) return GL_ERR_BAD_ARG;
    const size_t lds = (size_t)(49 * DW_CC + 7 * DW_WIN * DW_CC + DW_TW * C) * sizeof(float);      // <= 62 208 B (C <= 768)
    dwconv_ln_kernel<<<dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream>>>(x, w, bias, ln_gamma, ln_beta, H, W, C, ldo,
                                                                                   reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sp_gelu(const void* x, void* y, int64_t n, void* stream) {
    if (!x || !y || n <= 0 || (n % 2) != 0 || n / 512 >= 0x7fffffff) return GL_ERR_BAD_ARG;
    gelu_kernel<<<dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(reinterpret_cast<const half_t*>(x),
                                                                                            reinterpret_cast<half_t*>(y), n);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sp_down_gather(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* ln_gamma, const float* ln_beta, void* out,
                                 void* stream) {
    if (!x || !ln_gamma || !ln_beta || !out || B <= 0 || H <= 0 || W <= 0 || (H % 2) != 0 || (W % 2) != 0 || C <= 0) return GL_ERR_BAD_ARG;
    const int64_t pix = (int64_t)B * H * W;
    if ((pix + 3) / 4 > 0x7fffffff) return GL_ERR_BAD_ARG;
    down_gather_kernel<<<dim3((unsigned)((pix + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(x, B, H, W, C, ln_gamma, ln_beta,
                                                                                             reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sp_assemble(const float* feat, const float* mask, const float* null_feature, const float* pos, int32_t B, int32_t T, int32_t C,
                              void* out, void* stream) {
    if (!feat || !mask || !null_feature || !pos || !out || B <= 0 || T <= 0 || C <= 0) return GL_ERR_BAD_ARG;
    assemble_kernel<<<dim3(B * T), dim3(256), 0, (hipStream_t)stream>>>(feat, mask, null_feature, pos, T, C, reinterpret_cast<half_t*>(out));
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sp_bicubic(const float* in, int32_t B, int32_t Ct, int32_t C, int32_t Hin, int32_t Win, const int32_t* iy, const float* wy,
                             const int32_t* ix, const float* wx, int32_t Hout, int32_t Wout, float* out, void* stream) {
    if (!in || !iy || !wy || !ix || !wx || !out || B <= 0 || C <= 0 || C > Ct || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return GL_ERR_BAD_ARG;
    const int64_t total = (int64_t)B * C * Hout * Wout;
    if ((total + 255) / 256 > 0x7fffffff) return GL_ERR_BAD_ARG;
    bicubic_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(in, Ct, C, Hin, Win, iy, wy, ix, wx, Hout, Wout, total,
                                                                                               out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sp_conv4x4s2(const float* in, const float* w, const float* bias, int32_t B, int32_t Ci, int32_t Co, int32_t Hin, int32_t Win,
                               int32_t silu, float* out, void* stream) {
    if (!in || !w || !bias || !out || B <= 0 || Ci <= 0 || Ci > 8 || Co <= 0 || Co > 8 || Hin <= 0 || Win <= 0 || (Hin % 2) != 0 || (Win % 2) != 0)
        return GL_ERR_BAD_ARG;
    const int64_t total = (int64_t)B * Co * (Hin / 2) * (Win / 2);
    if ((total + 255) / 256 > 0x7fffffff) return GL_ERR_BAD_ARG;
    conv4x4s2_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(in, w, bias, Ci, Co, Hin, Win, silu, total, out);
    GL_CHECK_LAUNCH();
    return 0;
}
