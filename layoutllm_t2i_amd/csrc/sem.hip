// Kernels of the semantic-map grounding family (GLIGEN's checkpoint_generation_sem.pth): the front end that sem_grounding_net.PositionNet and
// sem_grounding_downsampler.GroundingDownsampler put before the ConvNeXt / the first conv.  The reference feeds both a fp32 one-hot tensor
// [B, classes, 512, 512] (159 MB per sample at 152 classes), resizes it (nearest) and convolves it.  A convolution over a one-hot input is a
// table lookup,
//   out[co, y, x] = bias[co] + sum over in-bounds taps (ky, kx) of W[co, class(y * s - p + ky, x * s - p + kx), ky, kx],
// so the input here is the uint8 CLASS MAP [B, Hs, Ws] and the one-hot tensor is never built.  Everything runs ONCE per image:
//   gl_sem_gather_conv    nearest resize to R x R + K x K / stride / pad conv as a weight gather (+ SiLU), fp32 NCHW out
//   gl_sem_conv4x4s2      the downsampler's second conv, Conv2d(Ci <= 64, Co <= 64, 4, 2, 1), fp32 FMA
//   gl_sem_onehot_index   fp32 one-hot [B, C, H, W] -> uint8 class map + a per-sample count of pixels that are not exactly one-hot
// Plain HIP C++, vector stores only.
#include "common.h"
#include "gligen_hip.h"

namespace {

// F.interpolate(mode="nearest"): src = min(floor(dst * (float)in / out), in - 1), the scale in fp32 as torch computes it (spatial.hip)
__device__ __forceinline__ int nearest_src(int dst, int in, int out) {
    const int s = (int)floorf((float)dst * ((float)in / (float)out));
    return s < in - 1 ? s : in - 1;
}

// One thread per output pixel (b, oy, ox), all Co channels: per in-bounds tap one class id (a byte of the map, through the nearest resize) and
// NV dwordx4 loads of the table row [class][tap][4 NV] (Co padded to 4 NV floats, the pad zero).  The table is NOT staged in LDS: it is read by
// every block and stays in L2 (21 888 B for the tokenizer's 3x3, 155 648 B for the downsampler's 4x4 at 152 classes), a block of 256 pixels
// needs at most 256 x K^2 rows of it while staging would read all of it per block and leave one block per CU; neighbouring pixels of a
// segmentation map mostly share a class, so the lanes of a wave mostly read the same row.  Stores are coalesced along ox per channel.
// A class id >= classes (refused on the host) is clamped, so no read leaves the table.
template <int NV>
__global__ __launch_bounds__(256) void gather_conv_kernel(const uint8_t* __restrict__ map, int Hs, int Ws, int R, const f32x4* __restrict__ table,
                                                          const float* __restrict__ bias, int classes, int K, int stride, int pad, int Co, int Ro,
                                                          int silu, int64_t total, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % Ro);
    const int oy = (int)((idx / Ro) % Ro);
    const int b = (int)(idx / ((int64_t)Ro * Ro));
    const uint8_t* m = map + (size_t)b * Hs * Ws;
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < K; ++ky) {
        const int y = oy * stride - pad + ky;
        if (y < 0 || y >= R) continue;                   // zero padding of a one-hot: no class, nothing to add
        const uint8_t* row = m + (size_t)nearest_src(y, Hs, R) * Ws;
        for (int kx = 0; kx < K; ++kx) {
            const int x = ox * stride - pad + kx;
            if (x < 0 || x >= R) continue;
            int c = row[nearest_src(x, Ws, R)];
            c = c < classes ? c : classes - 1;
            const f32x4* t = table + ((size_t)c * K * K + ky * K + kx) * NV;
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] += t[v];
        }
    }
    const size_t plane = (size_t)Ro * Ro;
    float* o = out + (size_t)b * Co * plane + (size_t)oy * Ro + ox;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = v * 4 + j;
            if (co < Co) {
                const float a = acc[v][j] + bias[co];
                o[co * plane] = silu ? a / (1.0f + expf(-a)) : a;
            }
        }
    }
}

// Conv2d(Ci, Co, 4, 2, 1) on fp32 NCHW, one thread per output value (spatial.hip's conv4x4s2_kernel without its 8-channel limit)
__global__ __launch_bounds__(256) void sem_conv4x4s2_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                            int Ci, int Co, int Hin, int Win, int64_t total, float* __restrict__ out) {
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
    out[idx] = acc;
}

// One thread per pixel, grid (pixel blocks, B): the C channel values of a pixel are C planes apart, so consecutive lanes read consecutive
// addresses of every plane and each element is read once.  The index is torch.argmax's (the first maximum); a pixel is one-hot when exactly one
// channel is 1.0 and every other is 0.0 (a NaN is neither).  Bad pixels are rare: one vector atomic each on the sample's counter.
__global__ __launch_bounds__(256) void onehot_index_kernel(const float* __restrict__ x, int C, int HW, uint8_t* __restrict__ out,
                                                           int* __restrict__ bad) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int b = blockIdx.y;
    const float* s = x + (size_t)b * C * HW + p;
    float best = s[0];
    int arg = 0, ones = 0, other = 0;
    for (int c = 0; c < C; ++c) {
        const float v = s[(size_t)c * HW];
        if (v > best) { best = v; arg = c; }
        if (v == 1.0f) ++ones;
        else if (!(v == 0.0f)) ++other;
    }
    out[(size_t)b * HW + p] = (uint8_t)arg;
    if (ones != 1 || other != 0) atomicAdd(bad + b, 1);
}

}  // namespace

extern "C" int gl_sem_gather_conv(const uint8_t* map, int32_t B, int32_t Hs, int32_t Ws, int32_t R, const float* table, const float* bias,
                                  int32_t classes, int32_t K, int32_t stride, int32_t pad, int32_t Co, int32_t silu, float* out, void* stream) {
    if (!map || !table || !bias || !out || B <= 0 || Hs <= 0 || Ws <= 0 || R <= 0 || classes < 2 || classes > 256 || K < 1 || K > 4 ||
        (stride != 1 && stride != 2) || pad < 0 || pad >= K || Co < 1 || Co > 16 || R + 2 * pad < K || (stride == 2 && (R % 2) != 0) ||
        ((uintptr_t)table % 16) != 0)
        return GL_ERR_BAD_ARG;
    const int Ro = (R + 2 * pad - K) / stride + 1;
    const int64_t total = (int64_t)B * Ro * Ro;
    if ((total + 255) / 256 > 0x7fffffff) return GL_ERR_BAD_ARG;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const f32x4* t = reinterpret_cast<const f32x4*>(table);
    hipStream_t st = (hipStream_t)stream;
    switch ((Co + 3) / 4) {
        case 1: gather_conv_kernel<1><<<grid, block, 0, st>>>(map, Hs, Ws, R, t, bias, classes, K, stride, pad, Co, Ro, silu, total, out); break;
        case 2: gather_conv_kernel<2><<<grid, block, 0, st>>>(map, Hs, Ws, R, t, bias, classes, K, stride, pad, Co, Ro, silu, total, out); break;
        case 3: gather_conv_kernel<3><<<grid, block, 0, st>>>(map, Hs, Ws, R, t, bias, classes, K, stride, pad, Co, Ro, silu, total, out); break;
        default: gather_conv_kernel<4><<<grid, block, 0, st>>>(map, Hs, Ws, R, t, bias, classes, K, stride, pad, Co, Ro, silu, total, out); break;
    }
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sem_conv4x4s2(const float* in, const float* w, const float* bias, int32_t B, int32_t Ci, int32_t Co, int32_t Hin, int32_t Win,
                                float* out, void* stream) {
    if (!in || !w || !bias || !out || B <= 0 || Ci <= 0 || Ci > 64 || Co <= 0 || Co > 64 || Hin <= 0 || Win <= 0 || (Hin % 2) != 0 || (Win % 2) != 0)
        return GL_ERR_BAD_ARG;
    const int64_t total = (int64_t)B * Co * (Hin / 2) * (Win / 2);
    if ((total + 255) / 256 > 0x7fffffff) return GL_ERR_BAD_ARG;
    sem_conv4x4s2_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(in, w, bias, Ci, Co, Hin, Win, total, out);
    GL_CHECK_LAUNCH();
    return 0;
}

extern "C" int gl_sem_onehot_index(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, uint8_t* out, int32_t* bad, void* stream) {
    if (!x || !out || !bad || B <= 0 || B > 65535 || C < 2 || C > 256 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffff - 256) return GL_ERR_BAD_ARG;
    const int HW = H * W;
    if (hipMemsetAsync(bad, 0, (size_t)B * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return GL_ERR_BAD_ARG;
    onehot_index_kernel<<<dim3((unsigned)((HW + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream>>>(x, C, HW, out, bad);
    GL_CHECK_LAUNCH();
    return 0;
}
