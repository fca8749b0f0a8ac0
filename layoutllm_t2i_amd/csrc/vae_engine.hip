// VAE decode stage behind the forward-level C ABI: gl_vae_create / gl_vae_load_weights / gl_vae_decode.
//
// Replaces AutoencoderKL.decode (GLIGEN/ldm/models/autoencoder.py:40-44) and Decoder.forward
// (GLIGEN/ldm/modules/diffusionmodules/model.py:535-568): z / scale_factor -> post_quant_conv (1x1, applied in fp32 while
// packing the latent) -> conv_in -> mid (ResnetBlock, single-head AttnBlock model.py:150-202, ResnetBlock) -> the up levels
// (num_res_blocks + 1 ResnetBlocks each, nearest-2x upsample + conv between levels) -> GroupNorm(eps 1e-6) + swish ->
// conv_out.  Like the UNet handle the engine owns the plan, the LIBRARY-DEFINED flat weight layout (gl_vae_weight_at: the
// host packer fills it, the same buffer travels in the multi-GPU broadcast), a grow-only activation pool with stable
// addresses and one hipGraph per (batch, latent rows, latent columns), captured on an engine-owned stream and replayed on the caller's.
// No new heavy kernels: every conv / 1x1 conv / GroupNorm goes through gl_conv3x3 / gl_gemm / gl_groupnorm (and therefore
// through the 8-wave deep-pipelined kernel wherever its dispatch applies).
//
// The same handle type also runs the ENCODE stage (gl_vae_encoder_create / gl_vae_encode): AutoencoderKL.encode
// (autoencoder.py:34-38) = Encoder.forward (model.py:368-459) -> quant_conv -> DiagonalGaussianDistribution.sample() * scale_factor,
// with the decoder's helpers (resnet, GroupNorm, conv, mid attention, pool, graphs); the two encoder-only pieces are the
// asymmetrically padded stride-2 Downsample (gl_conv3x3_pad01) and the posterior (gl_vae_posterior).
#include "common.h"
#include "gligen_hip.h"
#include "handle.h"
#include "opts.h"

#include <cstring>
#include <string>
#include <tuple>

namespace {
constexpr int VCIN_PAD = 64;
}  // namespace

struct gl_vae {
    gl_vae_config cfg;
    gl_weight_table wt;
    gl_pool pool;
    gl_graph_cache<std::tuple<int, int, int>> cache;      // (B, h, w)
    int launches = 0;
    gl_opt_overrides ovr;              // per-handle option overrides (gl_vae_set_option)
    bool fold_up = false;              // decoder: upsample convs stored as four folded 2x2 kernels [4 C, 4 C] (key 55 at gl_vae_create; gemm8.hip UPF)
    bool encoder = false;              // gl_vae_encoder_create: encode-stage plan (gl_vae_encode), else decode-stage (gl_vae_decode)

    // this handle has no error-string entry point: a refused pool request is the null pointer alone
    half_t* f16(const std::string& tag, size_t n) { return reinterpret_cast<half_t*>(pool.get(tag, n * 2, nullptr)); }
    float* f32(const std::string& tag, size_t n) { return reinterpret_cast<float*>(pool.get(tag, n * 4, nullptr)); }
};


namespace {

void plan_resnet(gl_vae* v, const std::string& p, int cin, int cout) {
    v->wt.add(p + ".norm1.g", 1, {cin}); v->wt.add(p + ".norm1.b", 1, {cin});
    v->wt.add(p + ".conv1.w", 0, {cout, 9 * (int64_t)cin}); v->wt.add(p + ".conv1.b", 1, {cout});
    v->wt.add(p + ".norm2.g", 1, {cout}); v->wt.add(p + ".norm2.b", 1, {cout});
    v->wt.add(p + ".conv2.w", 0, {cout, 9 * (int64_t)cout}); v->wt.add(p + ".conv2.b", 1, {cout});
    if (cin != cout) { v->wt.add(p + ".nin_shortcut.w", 0, {cout, cin}); v->wt.add(p + ".nin_shortcut.b", 1, {cout}); }
}

// pool tags of per-resolution buffers carry rows x columns: 8x12 and 12x8 are different levels
std::string lt(int h, int w) { return std::to_string(h) + "x" + std::to_string(w); }

struct VRun {
    gl_vae* v;
    hipStream_t st;
    int B;
    int* launches;
    void count(int n = 1) { if (launches) *launches += n; }
};

int v_gn(VRun& r, const half_t* x, int C, int HW, const std::string& p, bool silu, const std::string& tag, half_t** out) {
    gl_vae* v = r.v;
    const int nchunk = gn_nchunk(HW);
    float* partial = v->f32("gn.partial", (size_t)r.B * nchunk * 64);
    half_t* y = v->f16(tag, (size_t)r.B * HW * C);
    CKP(partial); CKP(y);
    CK(gl_groupnorm(x, C, nullptr, 0, r.B, HW, v->wt.ptr<float>(p + ".g"), v->wt.ptr<float>(p + ".b"), 1e-6f, silu ? 1 : 0, y, partial, nchunk, r.st));
    r.count(gl_groupnorm_launches(C, HW));
    *out = y;
    return 0;
}

// down != 0: the encoder's Downsample (F.pad(x, (0, 1, 0, 1)) + stride-2 pad-0 conv, gl_conv3x3_pad01), (h, w) -> (h / 2, w / 2)
int v_conv(VRun& r, const half_t* x, int sh, int sw, int cin, const std::string& p, int cout, int up, int epi, const void* res, void* out,
           int out_mode = GL_OUT_F16_ROWMAJOR, int down = 0) {
    gl_vae* v = r.v;
    gl_conv_args a;
    memset(&a, 0, sizeof(a));
    a.in = x;
    a.B = r.B; a.Hin = sh; a.Win = sw; a.Cin = cin;
    a.Hout = up ? 2 * sh : (down ? sh / 2 : sh);
    a.Wout = up ? 2 * sw : (down ? sw / 2 : sw);
    a.stride = down ? 2 : 1; a.upsample2x = up ? (v->fold_up ? 2 : 1) : 0;
    a.g.w = v->wt.ptr<half_t>(p + ".w");
    a.g.bias = v->wt.ptr<float>(p + ".b");
    a.g.N = cout;
    a.g.epi = epi;
    a.g.out_mode = out_mode;
    a.g.out = out;
    a.g.ldc = out_mode == GL_OUT_F32_NCHW ? 0 : cout;
    a.g.hw = out_mode == GL_OUT_F32_NCHW ? a.Hout * a.Wout : 0;
    a.g.res = res; a.g.ldres = cout;
    float* ws = v->f32("ws", (size_t)GL_WS_BYTES / 4);
    CKP(ws);
    a.g.workspace = ws; a.g.workspace_bytes = GL_WS_BYTES;
    CK(down ? gl_conv3x3_pad01(&a, r.st) : gl_conv3x3(&a, r.st));
    r.count();
    return 0;
}

int v_gemm(VRun& r, const half_t* a_, int lda, const half_t* w, const float* bias, int M, int N, int K, int epi, const void* res, half_t* out,
           int ldc) {
    gl_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.a = a_; g.lda = lda; g.w = w; g.bias = bias; g.M = M; g.N = N; g.K = K; g.epi = epi;
    g.out_mode = GL_OUT_F16_ROWMAJOR; g.out = out; g.ldc = ldc; g.res = res; g.ldres = N;
    float* ws = r.v->f32("ws", (size_t)GL_WS_BYTES / 4);
    CKP(ws);
    g.workspace = ws; g.workspace_bytes = GL_WS_BYTES;
    CK(gl_gemm(&g, r.st));
    r.count();
    return 0;
}

int v_resnet(VRun& r, const std::string& p, const half_t* x, int sh, int sw, int cin, int cout, const std::string& tag, half_t** out) {
    gl_vae* v = r.v;
    const int HW = sh * sw;
    const std::string ss = lt(sh, sw);
    const size_t M = (size_t)r.B * HW;
    half_t *t1, *t2;
    CK(v_gn(r, x, cin, HW, p + ".norm1", true, "rn.gn." + std::to_string(cin) + "." + ss, &t1));
    half_t* h = v->f16("rn.h." + std::to_string(cout) + "." + ss, M * cout);
    CKP(h);
    CK(v_conv(r, t1, sh, sw, cin, p + ".conv1", cout, 0, GL_EPI_BIAS, nullptr, h));
    CK(v_gn(r, h, cout, HW, p + ".norm2", true, "rn.gn." + std::to_string(cout) + "." + ss, &t2));
    const half_t* sk = x;
    if (cin != cout) {
        half_t* s = v->f16("rn.sk." + std::to_string(cout) + "." + ss, M * cout);
        CKP(s);
        CK(v_gemm(r, x, cin, v->wt.ptr<half_t>(p + ".nin_shortcut.w"), v->wt.ptr<float>(p + ".nin_shortcut.b"), (int)M, cout, cin, GL_EPI_BIAS, nullptr, s, cout));
        sk = s;
    }
    half_t* o = v->f16(tag, M * cout);
    CKP(o);
    CK(v_conv(r, t2, sh, sw, cout, p + ".conv2", cout, 0, GL_EPI_RES, sk, o));
    *out = o;
    return 0;
}

// single-head AttnBlock (model.py:150-202): d = C = 512 is beyond the flash kernel's register budget; Q.K^T (GEMM) -> row softmax
// -> P.V (GEMM against V^T), per sample; C^-0.5 is folded into the q weights at pack time
int v_attn(VRun& r, const std::string& p, const half_t* x, int N, int C, const std::string& tag, half_t** out) {
    gl_vae* v = r.v;
    const int B = r.B;
    const size_t M = (size_t)B * N;
    half_t* hn;
    CK(v_gn(r, x, C, N, p + ".norm", false, "at.gn", &hn));
    half_t *q = v->f16("at.q", M * C), *k = v->f16("at.k", M * C), *vv = v->f16("at.v", M * C), *o = v->f16("at.o", M * C);
    CKP(q); CKP(k); CKP(vv); CKP(o);
    CK(v_gemm(r, hn, C, v->wt.ptr<half_t>(p + ".q.w"), v->wt.ptr<float>(p + ".q.b"), (int)M, C, C, GL_EPI_BIAS, nullptr, q, C));
    CK(v_gemm(r, hn, C, v->wt.ptr<half_t>(p + ".k.w"), v->wt.ptr<float>(p + ".k.b"), (int)M, C, C, GL_EPI_BIAS, nullptr, k, C));
    CK(v_gemm(r, hn, C, v->wt.ptr<half_t>(p + ".v.w"), v->wt.ptr<float>(p + ".v.b"), (int)M, C, C, GL_EPI_BIAS, nullptr, vv, C));
    const int Np = (N + 63) / 64 * 64;
    const int Hs = 4;
    half_t* vt = v->f16("at.vt", (size_t)B * C * Np);
    half_t* s = v->f16("at.s", (size_t)B * N * Np);
    CKP(vt); CKP(s);
    CK(gl_transpose_v(vv, (int64_t)N * C, C, vt, Np, B, Hs, C / Hs, N, r.st));
    r.count();
    if (Np != N) {
        if (hipMemsetAsync(s, 0, (size_t)B * N * Np * 2, r.st) != hipSuccess) return GL_ERR_BAD_ARG;
    }
    for (int b = 0; b < B; ++b) {
        half_t* sb = s + (size_t)b * N * Np;
        CK(v_gemm(r, q + (size_t)b * N * C, C, k + (size_t)b * N * C, nullptr, N, N, C, GL_EPI_BIAS, nullptr, sb, Np));
        CK(gl_softmax_rows(sb, N, N, Np, 1.0f, r.st));
        r.count();
        CK(v_gemm(r, sb, Np, vt + (size_t)b * C * Np, nullptr, N, C, Np, GL_EPI_BIAS, nullptr, o + (size_t)b * N * C, C));
    }
    half_t* y = v->f16(tag, M * C);
    CKP(y);
    CK(v_gemm(r, o, C, v->wt.ptr<half_t>(p + ".proj_out.w"), v->wt.ptr<float>(p + ".proj_out.b"), (int)M, C, C, GL_EPI_RES, x, y, C));
    *out = y;
    return 0;
}

int launch_decode(gl_vae* v, int B, int sh, int sw, hipStream_t st, int* launches) {
    const gl_vae_config& c = v->cfg;
    VRun r{v, st, B, launches};
    if (launches) *launches = 0;
    const int nres = c.n_mult;
    int ch = c.ch * c.ch_mult[nres - 1];
    const float* z = v->f32("in.z", (size_t)B * c.z_channels * sh * sw);
    CKP(z);
    half_t* xin = v->f16("in", (size_t)B * sh * sw * VCIN_PAD);
    CKP(xin);
    CK(gl_latent_affine_pack(z, v->wt.ptr<float>("post_quant_conv.w"), v->wt.ptr<float>("post_quant_conv.b"), 1.0f / c.scale_factor, B, c.z_channels,
                              sh * sw, VCIN_PAD, xin, st));
    r.count();
    half_t* h = v->f16("conv_in", (size_t)B * sh * sw * ch);
    CKP(h);
    CK(v_conv(r, xin, sh, sw, VCIN_PAD, "decoder.conv_in", ch, 0, GL_EPI_BIAS, nullptr, h));
    CK(v_resnet(r, "decoder.mid.block_1", h, sh, sw, ch, ch, "mid.1", &h));
    CK(v_attn(r, "decoder.mid.attn_1", h, sh * sw, ch, "mid.a", &h));
    CK(v_resnet(r, "decoder.mid.block_2", h, sh, sw, ch, ch, "mid.2", &h));
    for (int lvl = nres - 1; lvl >= 0; --lvl) {
        const int cout = c.ch * c.ch_mult[lvl];
        for (int i = 0; i <= c.num_res_blocks; ++i) {
            CK(v_resnet(r, "decoder.up." + std::to_string(lvl) + ".block." + std::to_string(i), h, sh, sw, ch, cout,
                         "up." + std::to_string(lvl) + "." + std::to_string(i), &h));
            ch = cout;
        }
        if (lvl != 0) {
            half_t* u = v->f16("up." + std::to_string(lvl) + ".u", (size_t)B * 4 * sh * sw * ch);
            CKP(u);
            CK(v_conv(r, h, sh, sw, ch, "decoder.up." + std::to_string(lvl) + ".upsample.conv", ch, 1, GL_EPI_BIAS, nullptr, u));
            h = u;
            sh *= 2; sw *= 2;
        }
    }
    half_t* g;
    CK(v_gn(r, h, ch, sh * sw, "decoder.norm_out", true, "fin.gn", &g));
    float* out = v->f32("out", (size_t)B * c.out_ch * sh * sw);
    CKP(out);
    CK(v_conv(r, g, sh, sw, ch, "decoder.conv_out", c.out_ch, 0, GL_EPI_BIAS, nullptr, out, GL_OUT_F32_NCHW));
    return 0;
}

// Encoder.forward (model.py:428-459) + quant_conv + posterior sample: x fp32 NCHW image ("in.x") -> z fp32 NCHW ("out.z")
int launch_encode(gl_vae* v, int B, int sh, int sw, hipStream_t st, int* launches) {
    const gl_vae_config& c = v->cfg;
    VRun r{v, st, B, launches};
    if (launches) *launches = 0;
    const int nres = c.n_mult;
    const float* x = v->f32("in.x", (size_t)B * c.out_ch * sh * sw);
    half_t* xin = v->f16("in", (size_t)B * sh * sw * VCIN_PAD);
    CKP(x); CKP(xin);
    CK(gl_pack_latent(x, B, c.out_ch, sh * sw, VCIN_PAD, 1, 0, xin, st));
    r.count();
    int ch = c.ch;
    half_t* h = v->f16("conv_in", (size_t)B * sh * sw * ch);
    CKP(h);
    CK(v_conv(r, xin, sh, sw, VCIN_PAD, "encoder.conv_in", ch, 0, GL_EPI_BIAS, nullptr, h));
    for (int lvl = 0; lvl < nres; ++lvl) {
        const int cout = c.ch * c.ch_mult[lvl];
        for (int i = 0; i < c.num_res_blocks; ++i) {
            CK(v_resnet(r, "encoder.down." + std::to_string(lvl) + ".block." + std::to_string(i), h, sh, sw, ch, cout,
                         "down." + std::to_string(lvl) + "." + std::to_string(i), &h));
            ch = cout;
        }
        if (lvl != nres - 1) {
            half_t* d = v->f16("down." + std::to_string(lvl) + ".d", (size_t)B * (sh / 2) * (sw / 2) * ch);
            CKP(d);
            CK(v_conv(r, h, sh, sw, ch, "encoder.down." + std::to_string(lvl) + ".downsample.conv", ch, 0, GL_EPI_BIAS, nullptr, d,
                       GL_OUT_F16_ROWMAJOR, 1));
            h = d;
            sh /= 2; sw /= 2;
        }
    }
    CK(v_resnet(r, "encoder.mid.block_1", h, sh, sw, ch, ch, "mid.1", &h));
    CK(v_attn(r, "encoder.mid.attn_1", h, sh * sw, ch, "mid.a", &h));
    CK(v_resnet(r, "encoder.mid.block_2", h, sh, sw, ch, ch, "mid.2", &h));
    half_t* g;
    CK(v_gn(r, h, ch, sh * sw, "encoder.norm_out", true, "fin.gn", &g));
    const int hw = sh * sw, zc2 = 2 * c.z_channels;
    float* mom = v->f32("enc.h", (size_t)B * zc2 * hw);
    float* noise = v->f32("in.noise", (size_t)B * c.embed_dim * hw);
    float* z = v->f32("out.z", (size_t)B * c.embed_dim * hw);
    CKP(mom); CKP(noise); CKP(z);
    CK(v_conv(r, g, sh, sw, ch, "encoder.conv_out", zc2, 0, GL_EPI_BIAS, nullptr, mom, GL_OUT_F32_NCHW));
    CK(gl_vae_posterior(mom, v->wt.ptr<float>("quant_conv.w"), v->wt.ptr<float>("quant_conv.b"), noise, c.scale_factor, B, zc2, c.embed_dim, hw, z,
                         nullptr, st));
    r.count();
    return 0;
}

// What gl_vae_create and gl_vae_encoder_create both require; in_ch: the channels packed into the first conv's VCIN_PAD input channels
bool config_ok(const gl_vae_config* cfg, gl_vae** out, int in_ch) {
    return cfg && out && cfg->n_mult >= 1 && cfg->n_mult <= 8 && cfg->ch > 0 && (cfg->ch % 64) == 0 && cfg->num_res_blocks >= 0 && cfg->z_channels > 0 &&
           cfg->out_ch > 0 && in_ch <= VCIN_PAD && cfg->scale_factor != 0.0f;
}

// mid (model.py: ResnetBlock, single-head AttnBlock, ResnetBlock), p = "decoder.mid" / "encoder.mid"
void plan_mid(gl_vae* v, const std::string& p, int ch) {
    plan_resnet(v, p + ".block_1", ch, ch);
    const std::string ap = p + ".attn_1";
    v->wt.add(ap + ".norm.g", 1, {ch}); v->wt.add(ap + ".norm.b", 1, {ch});
    for (const char* n : {"q", "k", "v", "proj_out"}) { v->wt.add(ap + "." + n + ".w", 0, {ch, ch}); v->wt.add(ap + "." + n + ".b", 1, {ch}); }
    plan_resnet(v, p + ".block_2", ch, ch);
}

}  // namespace

extern "C" int gl_vae_create(const gl_vae_config* cfg, gl_vae** out) {
    if (!config_ok(cfg, out, cfg ? cfg->z_channels : 0)) return GL_ERR_BAD_ARG;
    gl_vae* v = new gl_vae();
    v->cfg = *cfg;
    v->fold_up = gl_opt(55) == 1;      // read ONCE: the weight table follows
    const int nres = cfg->n_mult;
    int ch = cfg->ch * cfg->ch_mult[nres - 1];
    v->wt.add("post_quant_conv.w", 1, {cfg->z_channels, cfg->embed_dim > 0 ? cfg->embed_dim : cfg->z_channels});
    v->wt.add("post_quant_conv.b", 1, {cfg->z_channels});
    v->wt.add("decoder.conv_in.w", 0, {ch, 9 * (int64_t)VCIN_PAD});
    v->wt.add("decoder.conv_in.b", 1, {ch});
    plan_mid(v, "decoder.mid", ch);
    for (int lvl = nres - 1; lvl >= 0; --lvl) {
        const int cout = cfg->ch * cfg->ch_mult[lvl];
        for (int i = 0; i <= cfg->num_res_blocks; ++i) {
            plan_resnet(v, "decoder.up." + std::to_string(lvl) + ".block." + std::to_string(i), ch, cout);
            ch = cout;
        }
        if (lvl != 0) {
            if (v->fold_up) v->wt.add("decoder.up." + std::to_string(lvl) + ".upsample.conv.w", 0, {4 * (int64_t)ch, 4 * (int64_t)ch});
            else v->wt.add("decoder.up." + std::to_string(lvl) + ".upsample.conv.w", 0, {ch, 9 * (int64_t)ch});
            v->wt.add("decoder.up." + std::to_string(lvl) + ".upsample.conv.b", 1, {ch});
        }
    }
    v->wt.add("decoder.norm_out.g", 1, {ch}); v->wt.add("decoder.norm_out.b", 1, {ch});
    v->wt.add("decoder.conv_out.w", 0, {cfg->out_ch, 9 * (int64_t)ch});
    v->wt.add("decoder.conv_out.b", 1, {cfg->out_ch});
    *out = v;
    return 0;
}

extern "C" int gl_vae_encoder_create(const gl_vae_config* cfg, gl_vae** out) {
    if (!config_ok(cfg, out, cfg ? cfg->out_ch : 0) || cfg->embed_dim <= 0) return GL_ERR_BAD_ARG;
    for (int l = 0; l < cfg->n_mult; ++l)
        if (cfg->ch_mult[l] <= 0) return GL_ERR_BAD_ARG;
    gl_vae* v = new gl_vae();
    v->cfg = *cfg;
    v->encoder = true;
    const int nres = cfg->n_mult;
    int ch = cfg->ch;
    v->wt.add("encoder.conv_in.w", 0, {ch, 9 * (int64_t)VCIN_PAD});
    v->wt.add("encoder.conv_in.b", 1, {ch});
    for (int lvl = 0; lvl < nres; ++lvl) {
        const int cout = cfg->ch * cfg->ch_mult[lvl];
        for (int i = 0; i < cfg->num_res_blocks; ++i) {
            plan_resnet(v, "encoder.down." + std::to_string(lvl) + ".block." + std::to_string(i), ch, cout);
            ch = cout;
        }
        if (lvl != nres - 1) {
            v->wt.add("encoder.down." + std::to_string(lvl) + ".downsample.conv.w", 0, {ch, 9 * (int64_t)ch});
            v->wt.add("encoder.down." + std::to_string(lvl) + ".downsample.conv.b", 1, {ch});
        }
    }
    plan_mid(v, "encoder.mid", ch);
    v->wt.add("encoder.norm_out.g", 1, {ch}); v->wt.add("encoder.norm_out.b", 1, {ch});
    v->wt.add("encoder.conv_out.w", 0, {2 * cfg->z_channels, 9 * (int64_t)ch});
    v->wt.add("encoder.conv_out.b", 1, {2 * cfg->z_channels});
    v->wt.add("quant_conv.w", 1, {2 * cfg->embed_dim, 2 * cfg->z_channels});
    v->wt.add("quant_conv.b", 1, {2 * cfg->embed_dim});
    *out = v;
    return 0;
}

extern "C" int gl_vae_encode(gl_vae* v, const float* x, int32_t B, int32_t side, const float* noise, float* z, int32_t use_graph, void* stream) {
    return gl_vae_encode_hw(v, x, B, side, side, noise, z, use_graph, stream);
}

extern "C" int gl_vae_encode_hw(gl_vae* v, const float* x, int32_t B, int32_t h, int32_t w, const float* noise, float* z, int32_t use_graph,
                                void* stream) {
    if (!v || !x || !noise || !z || B <= 0 || B >= 2048 || h <= 0 || h >= 1024 || w <= 0 || w >= 1024 || !v->wt.wbase || !v->encoder) return GL_ERR_BAD_ARG;
    const gl_vae_config& c = v->cfg;
    const int f = 1 << (c.n_mult - 1);
    if ((h % f) || (w % f)) return GL_ERR_BAD_ARG;
    gl_opts_scope opts_scope(v->ovr);
    hipStream_t st = (hipStream_t)stream;
    const size_t nx = (size_t)B * c.out_ch * h * w, nz = (size_t)B * c.embed_dim * (h / f) * (w / f);
    v->pool.changed = false;
    float* xin = v->f32("in.x", nx);
    float* nin = v->f32("in.noise", nz);
    float* zbuf = v->f32("out.z", nz);
    CKP(xin); CKP(nin); CKP(zbuf);
    if (hipMemcpyAsync(xin, x, nx * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    if (hipMemcpyAsync(nin, noise, nz * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    v->cache.sync_epochs(v->ovr);
    CK(v->cache.run(std::make_tuple((int)B, (int)h, (int)w), use_graph != 0, st, v->pool,
                    [&](hipStream_t s, int* nl) { return launch_encode(v, B, h, w, s, nl); }, &v->launches));
    if (hipMemcpyAsync(z, zbuf, nz * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    return 0;
}

extern "C" int gl_vae_destroy(gl_vae* v) {
    if (!v) return GL_ERR_BAD_ARG;
    v->cache.release();
    v->pool.release();
    delete v;
    return 0;
}

extern "C" int gl_vae_num_weights(const gl_vae* v) { return v ? (int)v->wt.names.size() : GL_ERR_BAD_ARG; }
extern "C" int64_t gl_vae_weights_bytes(const gl_vae* v) { return v ? v->wt.total : -1; }
extern "C" int gl_vae_weight_at(const gl_vae* v, int32_t i, gl_weight_info* info) { return v ? v->wt.info_at(i, info) : GL_ERR_BAD_ARG; }

extern "C" int gl_vae_load_weights(gl_vae* v, const void* packed, int64_t bytes, void* stream) {
    (void)stream;
    if (!v || !packed || bytes < v->wt.total || (reinterpret_cast<uintptr_t>(packed) % 16)) return GL_ERR_BAD_ARG;
    v->wt.wbase = reinterpret_cast<const char*>(packed);      // referenced, not copied: the caller keeps the buffer alive
    v->cache.drop();
    return 0;
}

extern "C" int gl_vae_decode(gl_vae* v, const float* z, int32_t B, int32_t side, float* out, int32_t use_graph, void* stream) {
    return gl_vae_decode_hw(v, z, B, side, side, out, use_graph, stream);
}

extern "C" int gl_vae_decode_hw(gl_vae* v, const float* z, int32_t B, int32_t h, int32_t w, float* out, int32_t use_graph, void* stream) {
    if (!v || !z || !out || B <= 0 || h <= 0 || w <= 0 || !v->wt.wbase || v->encoder) return GL_ERR_BAD_ARG;
    gl_opts_scope opts_scope(v->ovr);
    const gl_vae_config& c = v->cfg;
    hipStream_t st = (hipStream_t)stream;
    const size_t nz = (size_t)B * c.z_channels * h * w;
    const size_t f = (size_t)1 << (c.n_mult - 1);
    const size_t no = (size_t)B * c.out_ch * (f * h) * (f * w);
    v->pool.changed = false;
    float* zin = v->f32("in.z", nz);
    float* obuf = v->f32("out", no);
    CKP(zin); CKP(obuf);
    if (hipMemcpyAsync(zin, z, nz * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    v->cache.sync_epochs(v->ovr);
    CK(v->cache.run(std::make_tuple((int)B, (int)h, (int)w), use_graph != 0, st, v->pool,
                    [&](hipStream_t s, int* nl) { return launch_decode(v, B, h, w, s, nl); }, &v->launches));
    if (hipMemcpyAsync(out, obuf, no * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    return 0;
}

extern "C" int gl_vae_set_option(gl_vae* v, int key, int value) { return v ? gl_handle_set_option(v->ovr, key, value) : GL_ERR_BAD_ARG; }
extern "C" int gl_vae_num_launches(const gl_vae* v) { return v ? v->launches : GL_ERR_BAD_ARG; }
extern "C" int64_t gl_vae_pool_bytes(const gl_vae* v) { return v ? v->pool.bytes() : -1; }
extern "C" int gl_sizeof_vae_config(void) { return (int)sizeof(gl_vae_config); }
