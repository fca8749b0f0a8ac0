// Forward-level engine behind the C ABI: UNetModel.forward (openaimodel.py:413-459) and one PLMS step
// (plms.py:110-163) as a launch sequence over this library's kernels, with the block plan, the packed-weight
// layout, the activation pool, the hoisted conditioning and hipGraph capture / replay owned by one handle.
//
// What is result-identical restructuring of the reference (verified in tests/):
//   * token-major fp16 operands, fp32 residual stream: every block output / residual sum is produced in fp32 by the
//     GEMM / conv epilogue (+ an fp16 copy where a matrix-core consumer needs one);
//   * concat / residual / time-embedding / GEGLU / gates fused into GEMM and conv epilogues;
//   * conditioning-only work hoisted into gl_set_conditioning (once per image instead of 102 times);
//   * the gated self-attention fuser skipped outright at scale 0 (exact identity);
//   * RelationCrossAttention in closed form (rela.hip);
//   * one hipGraph per (shape, fuser on/off, first-conv variant), replayed per step.
#include "common.h"
#include "gligen_hip.h"
#include "handle.h"
#include "opts.h"

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>


namespace {

constexpr int CIN_PAD = 64;              // the 4-channel latent is zero-padded to one 64-channel K block
#define g_fuse_merge_ln gl_opt(25)  // default 1;                 // A/B knob (gl_set_option 25): rela_merge also writes LayerNorm(norm2) of its rows
#define g_fuse_vt gl_opt(21)  // default 1;                       // A/B knob (gl_set_option 21): V^T written by the QKV GEMM epilogue (1) or by gl_transpose_v (0)
#define g_force_fuser gl_opt(20)  // default 0;                   // test knob (gl_set_option 20): execute the fuser even at scale 0 (zero gates)
#define g_precise gl_opt(41)      // default 1;                   // split-fp16 activations for the 1x1 convs + GroupNorm on the fp32 stream
#define g_h1_f32 gl_opt(42)       // default 1;                   // with key 41: the ResBlock's first conv writes fp32 for out_layers' GroupNorm
#define g_rela_compact gl_opt(43) // default 1;                   // the relation chain runs on max_b nvalid[b] (rounded up to 8) rows per sample instead of max_objs = 30
#define g_w3 gl_opt(45)          // default 1024;                // with key 41: the 1x1 convs' third pass xhi.Wlo (weights stored [Whi | Wlo]) for launches of more than this many rows (>= 1024; 0 = off)
#define g_in_split gl_opt(38)     // default 1;                   // the first conv's input as [hi | lo | hi] channels against [Whi | Whi | Wlo] weights (free: 4 of 64 padded channels are used)
#define g_strict gl_opt(50)       // default 0;                   // STRICT mode (handles created with split_weights): every matrix product takes split-fp16
                                                                  // operands -- activations [hi | lo] against the weight, + a third pass hi.Wlo with key 51 --
                                                                  // so that the forward reproduces the fp32 reference within north_star's rtol 1e-3 / atol 1e-4
#define g_strict_w3 gl_opt(51)    // default 1;                   // strict: the third pass x.Wlo (weights stored [Whi | Wlo])
#define g_share gl_opt(44)        // default 1;                   // 2B = [cond ; uncond] forwards: everything before the first conditioning-dependent op
                                                                  // (conv_in, the first ResBlock, proj_in .. attn1 of the first transformer) runs ONCE on
                                                                  // the B shared latents and is duplicated

enum Kind { CONV_IN = 0, RES = 1, ST = 2, DOWN = 3, UP = 4 };
struct LayerD {
    int kind;
    std::string prefix;
    int cin, cout, d_head;
};
struct BlockD {
    std::vector<LayerD> layers;
};
using WInfo = gl_weight_table::Entry;
// everything a captured launch sequence depends on besides the pool addresses and the option generation (which drop every graph)
struct GraphKey {
    int Bn, lat_h, lat_w, R, Lc;
    bool fuser_on, sd_conv;
    int reps;
    bool uniform_t;             // one timestep for the whole batch: with reps == 2 the shared cond / uncond prefix
    int rel_slots;
    bool no_relation;           // a handle without the rela_fuse chain (gl_unet_config.no_relation): another launch sequence
    auto tie() const { return std::tie(Bn, lat_h, lat_w, R, Lc, fuser_on, sd_conv, reps, uniform_t, rel_slots, no_relation); }
    bool operator<(const GraphKey& o) const { return tie() < o.tie(); }
};

__global__ void f32_to_f16_kernel(const float* __restrict__ x, half_t* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = (half_t)x[i];
}
__global__ void fill_f32_kernel(float* __restrict__ y, float v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = v;
}

// text_image PositionNet (text_image_grounding_net.py:60-62): the two MLP chains run chain-major ([2, B, n] rows); objs = cat([objs_text,
// objs_image], dim=1) is sample-major ([B, 2 n] rows).  Rows are copied as 32-bit words (fp16 rows have an even number of elements).
__global__ void cat_chains_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int B, int n, int words) {
    const size_t total = (size_t)2 * B * n * words;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int wd = (int)(i % words);
        const size_t row = i / words;               // (c * B + b) * n + k
        const int k = (int)(row % n);
        const size_t cb = row / n;
        const int b = (int)(cb % B), c = (int)(cb / B);
        dst[(((size_t)b * 2 + c) * n + k) * words + wd] = src[i];
    }
}

// Integer pixel rectangles of RelationCrossAttention.forward (attention.py:321-346) for one resolution, one thread per
// sample (the `break` at the first padded or degenerate box is sequential).  Arithmetic mirrors the reference exactly:
// float32 multiply by the python int, truncation toward zero (.to(torch.int)), x1 / y1 clamped with torch.minimum,
// x0 / y0 not clamped, then python slice semantics (negative indices wrap once, then clamp).  rects = (top, bottom, left,
// right) of the EFFECTIVE slice; poison = 1 where a used box has an empty slice (torch.mean of nothing = NaN).
#pragma clang fp contract(off)
__device__ __forceinline__ void py_slice(int start, int stop, int len, int* s, int* e) {
    if (start < 0) { start += len; if (start < 0) start = 0; } else if (start > len) start = len;
    if (stop < 0) { stop += len; if (stop < 0) stop = 0; } else if (stop > len) stop = len;
    *s = start;
    *e = stop > start ? stop : start;
}
__global__ void rela_rects_kernel(const float* __restrict__ boxes, const float* __restrict__ masks, int B, int n, int h, int w,
                                  int* __restrict__ rects, int* __restrict__ nvalid, int* __restrict__ poison) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B) return;
    float count = 0.0f;
    for (int i = 0; i < n; ++i) count += masks[(size_t)k * n + i];
    int nv = 0, bad = 0;
    bool open = true;
    for (int i = 0; i < n; ++i) {
        int* r = rects + ((size_t)k * n + i) * 4;
        r[0] = r[1] = r[2] = r[3] = 0;
        if (!open) continue;
        const float* bx = boxes + ((size_t)k * n + i) * 4;
        const int left = (int)(bx[0] * (float)w);
        const int top = (int)(bx[1] * (float)h);
        const int right = (int)fminf(bx[2] * (float)w, (float)w);
        const int bottom = (int)fminf(bx[3] * (float)h, (float)h);
        if ((float)i < count && left != right && top != bottom) {
            int t, b, l, rr;
            py_slice(top, bottom, h, &t, &b);
            py_slice(left, right, w, &l, &rr);
            r[0] = t; r[1] = b; r[2] = l; r[3] = rr;
            if ((b - t) * (rr - l) == 0) bad = 1;
            nv = i + 1;
        } else {
            open = false;
        }
    }
    nvalid[k] = nv;
    poison[k] = bad;
}
#pragma clang fp contract(fast)

}  // namespace

struct gl_engine {
    bool fold_up = false;              // upsample convs stored as four folded 2x2 kernels [4 Cout, 4 Cin]: key 55 at gl_create, never on a split_weights handle
    bool strict_hoists_ok = false;     // the strict-mode conditioning hoists match the current conditioning ...
    int strict_hoists_w3 = -1;         // ... and were computed under this value of key 51
    gl_unet_config cfg;
    std::vector<BlockD> input_blocks, output_blocks;
    BlockD middle;
    int out_channels_last = 0;
    std::vector<LayerD> st_layers;
    gl_weight_table wt;                // packed weights
    bool has_sd = false;
    std::unordered_map<std::string, int> emb_off;
    int emb_total = 0;
    std::vector<float> gate_tanh;      // [n_st][4]: fuser attn, fuser dense, rela attn, rela dense
    gl_pool pool;
    int device = -1;
    // conditioning
    bool cond_set = false;
    int Bn = 0, R = 0, Lc = 0, lat_h = 0, lat_w = 0;     // (lat_h, lat_w): the latent's rows and columns (gl_set_conditioning_hw)
    // inpaint_mode handles: the inpainting_extra_input [extra_bs, in_channels + 1, lat_h, lat_w] lives in the pool buffer "in.extra" (gl_set_inpaint_extra)
    bool extra_set = false;
    // spatial handles (grounding = 4): output channels of the grounding downsampler the GLIGEN first conv also reads (gl_set_extra_channels)
    int ground_extra = 0;
    int extra_bs = 0;
    gl_graph_cache<GraphKey> cache;
    float fuser_scale_cur = -1e30f;
    std::vector<float> gate_host;      // the [n_st][4] array last computed
    float* gate_pin[2] = {nullptr, nullptr};           // pinned double buffer the async upload reads from
    hipEvent_t gate_pin_ev[2] = {nullptr, nullptr};    // completion of the upload that used the slot
    bool gate_pin_used[2] = {false, false};
    size_t gate_pin_bytes = 0;
    int gate_pin_next = 0;
    int launches = 0;
    int rel_slots = 0;                 // rows per sample of the relation chain (gl_set_conditioning: max nvalid over samples and levels, rounded up to 8)
    gl_opt_overrides ovr;              // per-handle option overrides (gl_set_handle_option)
    std::string err;

    // ------------------------------------------------------------------ helpers
    const WInfo* wi(const std::string& n) const { return wt.find(n); }
    const void* W(const std::string& n) const { return wt.ptr<void>(n); }
    const float* Wf(const std::string& n) const { return wt.ptr<float>(n); }
    void* buf(const std::string& tag, size_t bytes) { return pool.get(tag, bytes, &err); }
    half_t* h16(const std::string& tag, size_t n) { return reinterpret_cast<half_t*>(buf(tag, n * 2)); }
    float* f32(const std::string& tag, size_t n) { return reinterpret_cast<float*>(buf(tag, n * 4)); }
};

namespace {

void add_w(gl_engine* e, const std::string& name, int dtype, std::initializer_list<int64_t> shape) { e->wt.add(name, dtype, shape); }
// a matrix [n, k]: with cfg.split_weights stored as rows [Whi | Wlo] (k columns each)
void add_mat(gl_engine* e, const std::string& name, int64_t n, int64_t k) {
    add_w(e, name, 0, {n, e->cfg.split_weights ? 2 * k : k});
}
void add_lin(gl_engine* e, const std::string& p, int64_t n, int64_t k, bool bias = true) {
    add_mat(e, p + ".w", n, k);
    if (bias) add_w(e, p + ".b", 1, {n});
}
// the three kinds of 1x1 conv (skip_connection, proj_in, proj_out): weight rows [Whi | Wlo], Whi = fp16(W), Wlo = fp16(W - Whi)
void add_lin_split(gl_engine* e, const std::string& p, int64_t n, int64_t k) {
    add_w(e, p + ".w", 0, {n, 2 * k});
    add_w(e, p + ".b", 1, {n});
}
void add_norm(gl_engine* e, const std::string& p, int64_t c) {
    add_w(e, p + ".g", 1, {c});
    add_w(e, p + ".b", 1, {c});
}
// (the first conv keeps its own split form inside its padded input channels: split = false)
void add_conv3(gl_engine* e, const std::string& p, int64_t cin, int64_t cout, bool split = true) {
    add_w(e, p + ".w", 0, {cout, (split && e->cfg.split_weights ? 18 : 9) * cin});
    add_w(e, p + ".b", 1, {cout});
}
void add_ff(gl_engine* e, const std::string& p, int64_t C) {
    add_mat(e, p + ".ff1.w", 8 * C, C);
    add_w(e, p + ".ff1.b", 1, {8 * C});
    add_lin(e, p + ".ff2", C, 4 * C);
}

// UNetModel.__init__ (openaimodel.py:290-391) as data; mirrors arch.build_plan
void build_plan(gl_engine* e) {
    const gl_unet_config& c = e->cfg;
    const int mc = c.model_channels, heads = c.num_heads;
    auto has_attn = [&](int ds) {
        for (int i = 0; i < c.n_attn_res; ++i) if (c.attention_resolutions[i] == ds) return true;
        return false;
    };
    e->input_blocks.push_back(BlockD{{LayerD{CONV_IN, "input_blocks.0.0", c.in_channels, mc, 0}}});
    std::vector<int> chans{mc};
    int ch = mc, ds = 1;
    for (int level = 0; level < c.n_levels; ++level) {
        const int mult = c.channel_mult[level];
        for (int r = 0; r < c.num_res_blocks; ++r) {
            const int idx = (int)e->input_blocks.size();
            BlockD b;
            b.layers.push_back(LayerD{RES, "input_blocks." + std::to_string(idx) + ".0", ch, mult * mc, 0});
            ch = mult * mc;
            if (has_attn(ds)) b.layers.push_back(LayerD{ST, "input_blocks." + std::to_string(idx) + ".1", ch, ch, ch / heads});
            e->input_blocks.push_back(b);
            chans.push_back(ch);
        }
        if (level != c.n_levels - 1) {
            const int idx = (int)e->input_blocks.size();
            e->input_blocks.push_back(BlockD{{LayerD{DOWN, "input_blocks." + std::to_string(idx) + ".0.op", ch, ch, 0}}});
            chans.push_back(ch);
            ds *= 2;
        }
    }
    e->middle.layers = {LayerD{RES, "middle_block.0", ch, ch, 0}, LayerD{ST, "middle_block.1", ch, ch, ch / heads},
                        LayerD{RES, "middle_block.2", ch, ch, 0}};
    for (int level = c.n_levels - 1; level >= 0; --level) {
        const int mult = c.channel_mult[level];
        for (int i = 0; i <= c.num_res_blocks; ++i) {
            const int ich = chans.back();
            chans.pop_back();
            const int idx = (int)e->output_blocks.size();
            BlockD b;
            b.layers.push_back(LayerD{RES, "output_blocks." + std::to_string(idx) + ".0", ch + ich, mc * mult, 0});
            ch = mc * mult;
            if (has_attn(ds)) b.layers.push_back(LayerD{ST, "output_blocks." + std::to_string(idx) + ".1", ch, ch, ch / heads});
            if (level && i == c.num_res_blocks) {
                b.layers.push_back(LayerD{UP, "output_blocks." + std::to_string(idx) + "." + std::to_string(b.layers.size()) + ".conv", ch, ch, 0});
                ds /= 2;
            }
            e->output_blocks.push_back(b);
        }
    }
    e->out_channels_last = ch;
}

template <class F>
void for_all_layers(gl_engine* e, F f) {
    for (auto& b : e->input_blocks) for (auto& l : b.layers) f(l);
    for (auto& l : e->middle.layers) f(l);
    for (auto& b : e->output_blocks) for (auto& l : b.layers) f(l);
}

// row width of the PositionNet's MLP input = K of its first layer: in_dim + 8 F Fourier features of a box (a multiple of 64, gl_create), or on a
// keypoint handle D + 4 F of an xy pair rounded UP to a multiple of 64 (the input kernel writes the pad columns, the table pads the weight)
inline int pin_width(const gl_unet_config& c) {
    return c.grounding == 2 ? (c.pos_in_dim + 4 * c.fourier_freqs + 63) / 64 * 64 : c.pos_in_dim + 8 * c.fourier_freqs;
}

// the packed-weight table, in the order weights.pack_state_dict produces its tensors
void build_table(gl_engine* e) {
    const gl_unet_config& c = e->cfg;
    const int mc = c.model_channels, te = 4 * mc, ctx = c.context_dim;
    add_lin(e, "time_embed.0", te, mc);
    add_lin(e, "time_embed.2", te, te);
    add_conv3(e, "input_blocks.0.0", CIN_PAD, mc, false);
    if (!c.inpaint_mode) add_conv3(e, "sd_first_conv", CIN_PAD, mc, false);       // (an inpaint_mode first conv is not restorable, openaimodel.py:296)
    int off = 0;
    for_all_layers(e, [&](LayerD& l) {
        const std::string& p = l.prefix;
        if (l.kind == UP && e->fold_up) {
            // nearest-2x + 3x3 as one 2x2 conv per output parity (weights.pack_conv_upfold): rows (parity, Cout), K = (channel block, tap, channel)
            add_w(e, p + ".w", 0, {4 * (int64_t)l.cout, 4 * (int64_t)l.cin});
            add_w(e, p + ".b", 1, {l.cout});
        } else if (l.kind == DOWN || l.kind == UP) {
            add_conv3(e, p, l.cin, l.cout);
        } else if (l.kind == RES) {
            add_norm(e, p + ".in_layers.0", l.cin);
            add_conv3(e, p + ".in_layers.2", l.cin, l.cout);
            add_norm(e, p + ".out_layers.0", l.cout);
            add_conv3(e, p + ".out_layers.3", l.cout, l.cout);
            if (l.cin != l.cout) add_lin_split(e, p + ".skip_connection", l.cout, l.cin);
            e->emb_off[p] = off;
            off += l.cout;
        } else if (l.kind == ST) {
            const int C = l.cin;
            e->st_layers.push_back(l);
            add_norm(e, p + ".norm", C);
            add_lin_split(e, p + ".proj_in", C, C);
            add_lin_split(e, p + ".proj_out", C, C);
            const std::string t = p + ".transformer_blocks.0";
            add_mat(e, t + ".attn1.qkv.w", 3 * C, C);
            add_lin(e, t + ".attn1.o", C, C);
            add_mat(e, t + ".attn2.q.w", C, C);
            add_mat(e, t + ".attn2.kv.w", 2 * C, ctx);
            add_lin(e, t + ".attn2.o", C, C);
            add_ff(e, t + ".ff", C);
            for (const char* n : {".norm1", ".norm2", ".norm3"}) add_norm(e, t + n, C);
            const std::string f = t + ".fuser";
            add_lin(e, f + ".linear", C, ctx);
            add_mat(e, f + ".attn.qkv.w", 3 * C, C);
            add_lin(e, f + ".attn.o", C, C);
            add_ff(e, f + ".ff", C);
            add_norm(e, f + ".norm1", C);
            add_norm(e, f + ".norm2", C);
            add_w(e, f + ".tanh_attn", 1, {1});
            add_w(e, f + ".tanh_dense", 1, {1});
            if (c.no_relation) return;      // the upstream block (attention_original.py:312-316) has no rela_fuse
            const std::string r = t + ".rela_fuse";
            add_mat(e, r + ".attn.q.w", C, C);
            add_mat(e, r + ".attn.kv.w", 2 * C, ctx);
            add_lin(e, r + ".attn.o", C, C);
            add_ff(e, r + ".ff", C);
            for (const char* n : {".norm1", ".norm2", ".norm3"}) add_norm(e, r + n, C);
            add_w(e, r + ".tanh_attn", 1, {1});
            add_w(e, r + ".tanh_dense", 1, {1});
        }
    });
    e->emb_total = off;
    add_lin(e, "emb_all", off, te);
    add_norm(e, "out.0", e->out_channels_last);
    add_conv3(e, "out.2", e->out_channels_last, c.out_channels);
    if (c.grounding == 1) {
        // text_image PositionNet (text_image_grounding_net.py:19-38): two MLPs, three null features
        add_w(e, "position_net.null_text", 1, {c.pos_in_dim});
        add_w(e, "position_net.null_image", 1, {c.pos_in_dim});
        add_w(e, "position_net.null_xyxy", 1, {8 * c.fourier_freqs});
        for (const char* n : {"position_net.linears_text", "position_net.linears_image"}) {
            const std::string p = n;
            add_lin(e, p + ".0", 512, c.pos_in_dim + 8 * c.fourier_freqs);
            add_lin(e, p + ".2", 512, 512);
            add_lin(e, p + ".4", c.pos_out_dim, 512);
        }
        return;
    }
    if (c.grounding == 4) return;       // spatial: the ConvNeXt tokenizer runs outside the handle, which takes finished tokens (gl_set_conditioning_tokens)
    if (c.grounding == 2) {
        // keypoint PositionNet (keypoint_grounding_net.py:15-31): two learned tables and two null features (fp32: the input kernel sums and
        // blends them), one MLP whose first layer's K = D + 4 F is zero-padded to the GEMMs' multiple of 64 (800 -> 832)
        add_w(e, "position_net.person_emb", 1, {c.max_objs / 17, c.pos_in_dim});
        add_w(e, "position_net.keypoint_emb", 1, {17, c.pos_in_dim});
        add_w(e, "position_net.null_person", 1, {c.pos_in_dim});
        add_w(e, "position_net.null_xy", 1, {4 * c.fourier_freqs});
        add_lin(e, "position_net.linears.0", 512, pin_width(c));
        add_lin(e, "position_net.linears.2", 512, 512);
        add_lin(e, "position_net.linears.4", c.pos_out_dim, 512);
        return;
    }
    add_w(e, "position_net.null_pos", 1, {c.pos_in_dim});
    add_w(e, "position_net.null_xyxy", 1, {8 * c.fourier_freqs});
    add_lin(e, "position_net.linears.0", 512, c.pos_in_dim + 8 * c.fourier_freqs);
    add_lin(e, "position_net.linears.2", 512, 512);
    add_lin(e, "position_net.linears.4", c.pos_out_dim, 512);
}

// channels the GLIGEN first conv reads besides the latent: the masked latent and the mask of an inpaint_mode handle (openaimodel.py:293-299), or
// the grounding downsampler's output on a spatial handle (openaimodel_original.py: cat([x, downsample_net(grounding_extra_input)], 1))
inline int extra_channels(const gl_unet_config& c, int ground_extra = 0) { return c.inpaint_mode ? c.in_channels + 1 : ground_extra; }
// input channels of input_blocks.0.0
inline int first_conv_in(const gl_unet_config& c, int ground_extra = 0) { return c.in_channels + extra_channels(c, ground_extra); }
// grounding tokens per sample (the fuser's extra keys): max_objs for the text PositionNet, 2 * max_objs for text_image; a keypoint handle's
// max_objs already counts tokens (17 per person)
inline int n_ground(const gl_unet_config& c) { return c.grounding == 1 ? 2 * c.max_objs : c.max_objs; }

inline int vt_ld(int Nk) {
    // row stride (keys) of a V^T buffer: Nk rounded up to the 64-key tile, plus one tile when that is a multiple of 512
    // keys (a 1 KiB-multiple row stride maps the d rows of every V^T tile onto the same L1 sets: 307 vs 277 us at N = 4096)
    const int n = (Nk + 63) / 64 * 64;
    return (n % 512 == 0) ? n + 64 : n;
}
// the per-resolution conditioning buffers (cond.rects.* / nvalid.* / poison.*) are named by rows x columns: 64x96, 96x64 and 64x64 are three levels
inline std::string level_tag(int h, int w) { return std::to_string(h) + "x" + std::to_string(w); }

// the launch sequence of one forward / of the conditioning hoists
struct Run {
    gl_engine* e;
    hipStream_t st;
    void* ws;
    int launches = 0;

    // Launch operands.  The helpers below take a short positional core that says what the launch is; everything optional is a member of
    // a small options aggregate, named at the call site with designated initialisers (in declaration order).
    struct Act { const void* p = nullptr; int ld = 0; bool hilo = false; };       // activation rows; hilo: every row is [hi | lo] (ld >= 2 x width)
    struct Rows { const void* p = nullptr; int ld = 0; bool f32 = false; };       // fp32-or-fp16 rows: a residual, a normalisation's source
    template <class T>
    struct MatT { T* p; int64_t bs; int ld; T* lo = nullptr; };                   // an attention matrix: batch stride, row stride, lo half of a split one
    using Mat = MatT<const half_t>; using MatOut = MatT<half_t>;
    struct VtMat { const half_t* p; int ld; const half_t* lo = nullptr; };        // V^T of an attention ([B * H * d] rows of ld keys)
    // the transposed V tail of a fused QKV projection (gl_gemm_args.vt ...; vt_lo with a [hi | lo] output)
    struct VtTail { void* vt; void* vt_lo; int col0, rows, d, ld, H; };

    struct GemmOpt {
        bool bias = true;               // false: a projection without one (q, kv, qkv); true: the layer's p + ".b" must exist
        int out_mode = GL_OUT_F16_ROWMAJOR, epi = GL_EPI_BIAS;
        Rows res{};                     // GL_EPI_RES / GL_EPI_GATE_RES
        const float* gate = nullptr;
        void* out2 = nullptr; int ldc2 = 0;     // fp16 copy of an fp32 output
        Act a2{}; int ksplit = 0;               // second A source from K column ksplit on (a folded th.cat)
        bool wsplit = false;            // an add_lin_split matrix (rows [Whi | Wlo] in every table)
        const VtTail* tail = nullptr;
    };
    // out = epi(a . W(p + ".w")^T + W(p + ".b"))
    int gemm(Act a, const std::string& p, int M, void* out, int ldc, const GemmOpt& o) {
        const WInfo* wi = e->wi(p + ".w");
        if (!wi) return GL_ERR_BAD_ARG;
        gl_gemm_args g{};
        g.a = a.p; g.lda = a.ld; g.a2 = o.a2.p; g.lda2 = o.a2.ld; g.ksplit = o.ksplit;
        g.w = e->W(p + ".w"); g.bias = o.bias ? e->Wf(p + ".b") : nullptr;
        if (o.bias && !g.bias) return GL_ERR_BAD_ARG;
        g.M = M; g.N = (int)wi->shape[0]; g.K = (int)wi->shape[1];
        const bool strict = g_strict != 0 && e->cfg.split_weights;
        if (o.wsplit || e->cfg.split_weights) {         // weight rows [Whi | Wlo] (add_lin_split; every matrix of a split_weights table): the true K is half the stored row
            const int Kc = g.K / 2;
            g.ldw = g.K; g.K = Kc;                      // (fp16 rows: Whi alone, exactly what a compact handle computes)
            if (a.hilo) {       // x.W = xhi.Whi + xlo.Whi (+ xhi.Wlo: third K segment, A from the second source = the hi half again)
                g.kwrap = Kc; g.K = 2 * Kc;
                // default mode: the third pass belongs to the add_lin_split matrices alone (the three kinds of 1x1 conv, key 45) -- on a
                // split_weights handle every other matrix is read for its Whi half, exactly what a compact handle computes
                const bool third = strict ? (g_strict_w3 != 0) : (o.wsplit && g_w3 > 0 && M > (g_w3 < 1024 ? 1024 : g_w3));
                if (third) {
                    if (o.a2.p != nullptr) return GL_ERR_BAD_ARG;  // the third pass needs the second-source slot: a two-source A cannot take it
                    g.K = 3 * Kc; g.a2 = a.p; g.lda2 = a.ld; g.ksplit = 2 * Kc;
                }
            }
        } else if (a.hilo) {    // A = [hi | lo] of the activation, both halves against the same weight (gl_gemm_args.kwrap)
            g.kwrap = g.K; g.ldw = g.K; g.K = 2 * g.K;
        }
        g.epi = o.epi; g.out_mode = o.out_mode; g.out = out; g.ldc = ldc;
        g.res = o.res.p; g.ldres = o.res.ld; g.res_f32 = o.res.f32; g.gate = o.gate;
        g.out2 = o.out2; g.ldc2 = o.ldc2;
        if (o.tail) {
            const VtTail& t = *o.tail;
            g.vt = t.vt; g.vt_lo = t.vt_lo; g.vt_col0 = t.col0; g.vt_rows = t.rows; g.vt_d = t.d; g.vt_ld = t.ld; g.vt_H = t.H;
        }
        g.workspace = ws; g.workspace_bytes = GL_WS_BYTES;
        ++launches;
        return gl_gemm(&g, st);
    }
    int gemm(Act a, const std::string& p, int M, void* out, int ldc) { return gemm(a, p, M, out, ldc, GemmOpt{}); }

    struct RowBias { const void* p = nullptr; int ld = 0, rows_per_sample = 0; };   // GL_EPI_ROWBIAS: one bias row per sample (the emb_layers output)
    struct ConvOpt {
        int stride = 1, ups = 0, epi = GL_EPI_BIAS;     // ups: nearest-2x upsample folded into the gather
        Rows res{};
        RowBias rowbias{};
        void* out2 = nullptr;           // fp16 copy of an fp32 output
        int nchw_hw = 0;                // GL_OUT_F32_NCHW: pixels per sample
    };
    // 3x3 conv of layer p (weights p + ".w", p + ".b") over in = [B, H, W] pixel rows of in.ld channels ([hi | lo] halves of in.ld / 2 each when in.hilo)
    int conv(Act in, const std::string& p, int B, int Hin, int Win, void* out, int out_mode, const ConvOpt& o) {
        const WInfo* wi = e->wi(p + ".w");
        if (!wi) return GL_ERR_BAD_ARG;
        const int Cin = in.hilo ? in.ld / 2 : in.ld;
        gl_conv_args a{};
        // weight rows [Whi | Wlo] in a split_weights table (not the first conv, which is split inside its padded channels)
        a.w_split = wi->shape[1] == 18 * (int64_t)Cin;
        // strict: the input pixels are [hi | lo] rows (2 Cin channels); third pass hi.Wlo with key 51
        a.in_split = in.hilo ? ((a.w_split && g_strict_w3 != 0) ? 3 : 2) : 0;
        a.in = in.p; a.B = B; a.Hin = Hin; a.Win = Win; a.Cin = Cin;
        a.Hout = o.ups ? 2 * Hin : (Hin + 2 - 3) / o.stride + 1;
        a.Wout = o.ups ? 2 * Win : (Win + 2 - 3) / o.stride + 1;
        // an upsample conv of a folded table ([4 Cout, 4 Cin] rows, gl_engine.fold_up) takes the folded form of the kernel
        const bool folded = o.ups && wi->shape[1] == 4 * (int64_t)Cin;
        a.stride = o.stride; a.upsample2x = folded ? 2 : o.ups;
        a.g.w = e->W(p + ".w"); a.g.bias = e->Wf(p + ".b"); a.g.N = (int)(folded ? wi->shape[0] / 4 : wi->shape[0]);
        a.g.epi = o.epi; a.g.out_mode = out_mode; a.g.out = out; a.g.ldc = a.g.N; a.g.hw = o.nchw_hw;
        a.g.res = o.res.p; a.g.ldres = o.res.ld; a.g.res_f32 = o.res.f32;
        a.g.rowbias = o.rowbias.p; a.g.ld_rowbias = o.rowbias.ld; a.g.rows_per_sample = o.rowbias.rows_per_sample;
        a.g.rowbias_f32 = o.rowbias.p != nullptr && (g_precise != 0 || g_strict != 0);      // precise mode: the emb_layers output stays fp32
        a.g.out2 = o.out2; a.g.ldc2 = a.g.N;
        a.g.workspace = ws; a.g.workspace_bytes = GL_WS_BYTES;
        ++launches;
        return gl_conv3x3(&a, st);
    }

    enum LnFlags { LN_X_F32 = 1, LN_X2_F32 = 4, LN_Y_HILO = 8 };     // the flag word of gl_layernorm
    struct LnOpt {
        int rows_out = 0;               // rows per sample of y when it has more than x (the [x ; x2 ; pad] rows of the fuser); 0 = rows
        float* stats = nullptr;         // also writes the per-row (mean, rstd)
        Rows x2{}; int rows2 = 0;       // rows2 further rows per sample, normalised behind x's
        bool y_lo = false;              // y rows written as [hi | lo] (ldy >= 2 C): the split-fp16 operand of the projection that follows (strict mode)
    };
    // LayerNorm p over the e->Bn samples of x ([rows, C] each) into y.  ln, gn and attn take the batch from the handle: a half-batch section
    // (the shared cond / uncond prefix) must hold a BnScope around its calls, or they run the full batch
    int ln(Rows x, half_t* y, int ldy, const std::string& p, int rows, int C, const LnOpt& o) {
        const int flags = (x.f32 ? LN_X_F32 : 0) | (o.x2.f32 ? LN_X2_F32 : 0) | (o.y_lo ? LN_Y_HILO : 0);
        ++launches;
        return gl_layernorm(x.p, x.ld, flags, y, ldy, e->Wf(p + ".g"), e->Wf(p + ".b"), e->Bn, rows, o.rows_out ? o.rows_out : rows, 0, C, 1e-5f, o.stats,
                            o.x2.p, C, o.rows2, st);
    }
    int ln(Rows x, half_t* y, int ldy, const std::string& p, int rows, int C) { return ln(x, y, ldy, p, rows, C, LnOpt{}); }
    // fp32 rows -> fp16 [hi | lo] rows (strict mode: stream tensors entering a down / up conv, conditioning tensors)
    int split(const float* x, int64_t rows, int C, half_t* y) {
        ++launches;
        return gl_split_f32(x, C, rows, C, y, 2 * C, st);
    }
    struct GnOpt {
        const void* x2 = nullptr; int C2 = 0;   // second source of C2 channels, same element type as x (a folded th.cat)
        int ldo = 0;
        half_t* out_lo = nullptr;               // out_lo / raw: the split-fp16 side outputs of gl_groupnorm_ex
        half_t* raw = nullptr; int ldraw = 0;
    };
    // GroupNorm p (+ SiLU) over the e->Bn samples of x ([HW, x.ld] each; x.f32: an fp32 stream tensor)
    int gn(Rows x, int HW, const std::string& p, float eps, int silu, half_t* out, const GnOpt& o) {
        const int B = e->Bn, nchunk = gn_nchunk(HW);
        float* partial = e->f32("gn.partial", (size_t)B * nchunk * 64);
        CKP(partial);
        launches += gl_groupnorm_launches_ex(x.ld + o.C2, HW, x.f32);
        gl_gn_args a{};
        a.x1 = x.p; a.C1 = x.ld; a.x2 = o.x2; a.C2 = o.C2; a.x_f32 = x.f32; a.B = B; a.HW = HW;
        a.gamma = e->Wf(p + ".g"); a.beta = e->Wf(p + ".b"); a.eps = eps; a.silu = silu;
        a.out = out; a.ldo = o.ldo; a.out_lo = o.out_lo; a.raw = o.raw; a.ldraw = o.ldraw;
        a.partial = partial; a.nchunk = nchunk;
        return gl_groupnorm_ex(&a, st);
    }
    int gn(Rows x, int HW, const std::string& p, float eps, int silu, half_t* out) { return gn(x, HW, p, eps, silu, out, GnOpt{}); }
    // attention of the e->Bn samples' cfg.num_heads heads: q [Nq, H d] against k [Nk, H d] and V^T, split-fp16 where the lo halves are given
    int attn(Mat q, Mat k, VtMat vt, MatOut out, int d, int Nq, int Nk) {
        gl_attn_args a{};
        a.q_lo = q.lo; a.k_lo = k.lo; a.vt_lo = vt.lo; a.out_lo = out.lo;
        a.q = q.p; a.q_bstride = q.bs; a.ldq = q.ld; a.k = k.p; a.k_bstride = k.bs; a.ldk = k.ld; a.vt = vt.p; a.ldvt = vt.ld;
        a.out = out.p; a.o_bstride = out.bs; a.ldo = out.ld; a.B = e->Bn; a.H = e->cfg.num_heads; a.d = d; a.Nq = Nq; a.Nk = Nk;
        a.scale = 1.0f / sqrtf((float)d);
        a.q_prescaled = 1;      // weights.py folds d^-1/2 * log2(e) into every q projection
        ++launches;
        return gl_attention(&a, st);
    }
    // rows [0, n) of a row-major tensor copied to rows [n, 2n): the uncond half of a tensor computed once for both halves
    int dup_rows(void* base, size_t bytes_half) {
        ++launches;
        return hipMemcpyAsync(reinterpret_cast<char*>(base) + bytes_half, base, bytes_half, hipMemcpyDeviceToDevice, st) == hipSuccess ? 0 : GL_ERR_BAD_ARG;
    }
    int transpose_v(const half_t* v, int64_t vb, int ldv, half_t* vt, int ldvt, int B, int H, int d, int Nk) {
        ++launches;
        return gl_transpose_v(v, vb, ldv, vt, ldvt, B, H, d, Nk, st);
    }
};

struct BnScope {            // the engine's batch for the duration of a half-batch (shared cond / uncond) section
    gl_engine* e;
    int saved;
    BnScope(gl_engine* e_, int bn) : e(e_), saved(e_->Bn) { e->Bn = bn; }
    ~BnScope() { e->Bn = saved; }
};

struct Stream2 {            // a residual-stream tensor: fp32 master + fp16 copy for matrix-core consumers
    float* f = nullptr;
    half_t* h = nullptr;
};

int set_fuser_scale(gl_engine* e, float scale, hipStream_t st) {
    if (e->fuser_scale_cur == scale) return 0;
    const size_t n = e->st_layers.size();
    float* gates = e->f32("gates", n * 4);
    CKP(gates);
    e->gate_host.resize(n * 4);
    for (size_t i = 0; i < n; ++i) {
        e->gate_host[i * 4 + 0] = scale * e->gate_tanh[i * 4 + 0];
        e->gate_host[i * 4 + 1] = scale * e->gate_tanh[i * 4 + 1];
        e->gate_host[i * 4 + 2] = e->gate_tanh[i * 4 + 2];
        e->gate_host[i * 4 + 3] = e->gate_tanh[i * 4 + 3];
    }
    // Pinned, double-buffered staging: the async copy reads host memory when the stream gets there, and the stage-1 alpha ramp
    // can change the scale on consecutive steps, so the source of the copy in flight must not be overwritten by the next call
    // (a pageable source is NOT guaranteed to be staged before hipMemcpyAsync returns on every runtime path).
    const size_t bytes = n * 4 * sizeof(float);
    if (e->gate_pin_bytes < bytes) {
        for (int k = 0; k < 2; ++k) {
            if (e->gate_pin[k]) (void)hipHostFree(e->gate_pin[k]);
            e->gate_pin[k] = nullptr;
            if (hipHostMalloc(reinterpret_cast<void**>(&e->gate_pin[k]), bytes, hipHostMallocDefault) != hipSuccess) return GL_ERR_BAD_ARG;
            if (e->gate_pin_ev[k] == nullptr && hipEventCreateWithFlags(&e->gate_pin_ev[k], hipEventDisableTiming) != hipSuccess) return GL_ERR_BAD_ARG;
        }
        e->gate_pin_bytes = bytes;
        e->gate_pin_used[0] = e->gate_pin_used[1] = false;
    }
    const int slot = e->gate_pin_next;
    e->gate_pin_next ^= 1;
    if (e->gate_pin_used[slot] && hipEventSynchronize(e->gate_pin_ev[slot]) != hipSuccess) return GL_ERR_BAD_ARG;   // copy issued two calls ago
    memcpy(e->gate_pin[slot], e->gate_host.data(), bytes);
    if (hipMemcpyAsync(gates, e->gate_pin[slot], bytes, hipMemcpyHostToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    if (hipEventRecord(e->gate_pin_ev[slot], st) != hipSuccess) return GL_ERR_BAD_ARG;
    e->gate_pin_used[slot] = true;
    e->fuser_scale_cur = scale;
    return 0;
}

// self-attention over src [Bn * rows_per_b, C] (already normalised): QKV GEMM -> V^T -> flash attention
int self_attention(Run& r, const half_t* src, int rows_per_b, int Nq, int Nk, int C, int d, const std::string& wp, const std::string& tag,
                   half_t** out) {
    gl_engine* e = r.e;
    const int Bn = e->Bn, H = e->cfg.num_heads;
    if (g_strict != 0) {
        // strict: src rows are [hi | lo] (2 C); q | k | v leave the projection as [hi (3 C) | lo (3 C)] rows, V^T hi / lo through the
        // transpose kernel, split-fp16 attention, output rows [hi | lo] (2 C) for the to_out projection
        half_t* qkv = e->h16(tag + ".qkv", (size_t)Bn * rows_per_b * 6 * C);
        const int ldvt = vt_ld(Nk > rows_per_b ? Nk : rows_per_b);
        half_t* vt = e->h16(tag + ".vt", (size_t)2 * Bn * H * d * ldvt);
        half_t* vtl = vt + (size_t)Bn * H * d * ldvt;
        half_t* att = e->h16(tag + ".att", (size_t)Bn * Nq * 2 * C);
        CKP(qkv); CKP(vt); CKP(att);
        const int64_t bs = (int64_t)rows_per_b * 6 * C;
        int rc = GL_ERR_UNSUPPORTED;
        if (g_fuse_vt && (C % 64) == 0 && Bn * rows_per_b >= 256) {
            // the V third leaves the projection's epilogue directly as the two V^T operands (hi, lo) of the split attention (ABI 15); only the
            // 8-wave kernel implements that tail (GL_ERR_UNSUPPORTED otherwise: the transposes below)
            const Run::VtTail tail{vt, vtl, 2 * C, rows_per_b, d, ldvt, H};
            rc = r.gemm({src, 2 * C, true}, wp + ".qkv", Bn * rows_per_b, qkv, 6 * C, {.bias = false, .out_mode = GL_OUT_F16_HILO, .tail = &tail});
            if (rc != 0 && rc != GL_ERR_UNSUPPORTED) return rc;
            if (rc != 0) --r.launches;
        }
        if (rc != 0) {
            CK(r.gemm({src, 2 * C, true}, wp + ".qkv", Bn * rows_per_b, qkv, 6 * C, {.bias = false, .out_mode = GL_OUT_F16_HILO}));
            CK(r.transpose_v(qkv + 2 * C, bs, 6 * C, vt, ldvt, Bn, H, d, Nk));
            CK(r.transpose_v(qkv + 5 * C, bs, 6 * C, vtl, ldvt, Bn, H, d, Nk));
        }
        CK(r.attn({qkv, bs, 6 * C, qkv + 3 * C}, {qkv + C, bs, 6 * C, qkv + 4 * C}, {vt, ldvt, vtl}, {att, (int64_t)Nq * 2 * C, 2 * C, att + C}, d, Nq, Nk));
        *out = att;
        return 0;
    }
    half_t* qkv = e->h16(tag + ".qkv", (size_t)Bn * rows_per_b * 3 * C);
    const int ldvt = vt_ld(Nk > rows_per_b ? Nk : rows_per_b);      // the fused V^T tail writes one column per ROW (pad rows included)
    half_t* vt = e->h16(tag + ".vt", (size_t)Bn * H * d * ldvt);
    half_t* att = e->h16(tag + ".att", (size_t)Bn * Nq * C);
    CKP(qkv); CKP(vt); CKP(att);
    const int64_t bs = (int64_t)rows_per_b * 3 * C;
    // fused QKV projection; its V third is written directly as the attention kernel's V^T operand by the GEMM epilogue
    // when the V columns start on an epilogue pass of every tile shape (true for all widths of this UNet), else by the
    // separate transpose kernel
    if (g_fuse_vt && (C % 32) == 0) {
        const Run::VtTail tail{vt, nullptr, 2 * C, rows_per_b, d, ldvt, H};
        CK(r.gemm({src, C}, wp + ".qkv", Bn * rows_per_b, qkv, 3 * C, {.bias = false, .tail = &tail}));
    } else {
        CK(r.gemm({src, C}, wp + ".qkv", Bn * rows_per_b, qkv, 3 * C, {.bias = false}));
        CK(r.transpose_v(qkv + 2 * C, bs, 3 * C, vt, ldvt, Bn, H, d, Nk));
    }
    CK(r.attn({qkv, bs, 3 * C}, {qkv + C, bs, 3 * C}, {vt, ldvt}, {att, (int64_t)Nq * C, C}, d, Nq, Nk));
    *out = att;
    return 0;
}

int feed_forward(Run& r, const half_t* xn, const float* res, const std::string& p, int M, int C, void* out, int out_mode, const float* gate) {
    const int ldc = out_mode == GL_OUT_F16_HILO ? 2 * C : C;       // [hi | lo] rows for a split-fp16 consumer
    if (g_strict != 0) {
        // strict: xn rows are [hi | lo]; the GEGLU rows leave the first projection as [hi (4 C) | lo (4 C)]
        half_t* hg = r.e->h16("ff.h", (size_t)M * 8 * C);
        CKP(hg);
        CK(r.gemm({xn, 2 * C, true}, p + ".ff1", M, hg, 8 * C, {.out_mode = GL_OUT_F16_HILO, .epi = GL_EPI_GEGLU}));
        return r.gemm({hg, 8 * C, true}, p + ".ff2", M, out, ldc, {.out_mode = out_mode, .epi = gate ? GL_EPI_GATE_RES : GL_EPI_RES, .res = {res, C, true}, .gate = gate});
    }
    if (gl_ff_fused_applicable(C, M) && !r.e->cfg.split_weights) {
        // narrow / long level: the whole FeedForward in one launch, the [M, 4C] GEGLU intermediate never leaves the CU
        gl_ff_args a{};
        a.x = xn; a.ldx = C;
        a.w1 = r.e->W(p + ".ff1.w"); a.b1 = r.e->Wf(p + ".ff1.b");
        a.w2 = r.e->W(p + ".ff2.w"); a.b2 = r.e->Wf(p + ".ff2.b");
        if (!a.w1 || !a.b1 || !a.w2 || !a.b2) return GL_ERR_BAD_ARG;
        a.res = res; a.ldres = C; a.res_f32 = 1;
        a.gate = gate;
        a.out = out; a.ldc = ldc; a.out_mode = out_mode;
        a.M = M; a.C = C;
        ++r.launches;
        return gl_ff_fused(&a, r.st);
    }
    half_t* hg = r.e->h16("ff.h", (size_t)M * 4 * C);
    CKP(hg);
    CK(r.gemm({xn, C}, p + ".ff1", M, hg, 4 * C, {.epi = GL_EPI_GEGLU}));
    return r.gemm({hg, 4 * C}, p + ".ff2", M, out, ldc, {.out_mode = out_mode, .epi = gate ? GL_EPI_GATE_RES : GL_EPI_RES, .res = {res, C, true}, .gate = gate});
}

// ResBlock._forward (openaimodel.py:211-231); skip = the popped skip-stack tensor of an output block (th.cat folded in).
// need_h: the output also gets an fp16 copy (its consumer is a down / up conv, or the round-3 fp16-copy mode is on).
int res_block(Run& r, const LayerD& l, Stream2 h, const Stream2* skip, int skip_c, int sh, int sw, const void* emb_out, const std::string& tag,
              bool need_h, Stream2* out) {
    gl_engine* e = r.e;
    const int Bn = e->Bn, HW = sh * sw, M = Bn * HW;
    const std::string& p = l.prefix;
    const int c1 = l.cin - skip_c;
    const bool strict = g_strict != 0;
    const bool precise = g_precise != 0 || strict, h1f = precise && (g_h1_f32 != 0 || strict), has_skip_conv = l.cin != l.cout;
    // strict: both GroupNorm outputs are [hi | lo] pixel rows, the 3x3 convs take split-fp16 inputs
    half_t* t = e->h16("rb.gn1", (size_t)M * l.cin * (strict ? 2 : 1));
    half_t* t2 = e->h16("rb.gn2", (size_t)M * l.cout * (strict ? 2 : 1));
    CKP(t); CKP(t2);
    // in_layers GroupNorm + SiLU.  precise: reads the fp32 stream itself and, for a block with a 1x1 skip_connection, also writes
    // the raw input concat as [hi | lo] fp16 -- the split-fp16 operand of that 1x1 conv (its input IS the block input, :231)
    half_t* split = nullptr;
    if (precise) {
        if (has_skip_conv) { split = e->h16("rb.split", (size_t)M * 2 * l.cin); CKP(split); }
        CK(r.gn({h.f, c1, true}, HW, p + ".in_layers.0", 1e-5f, 1, t,
                {.x2 = skip ? skip->f : nullptr, .C2 = skip_c, .ldo = strict ? 2 * l.cin : 0, .out_lo = strict ? t + l.cin : nullptr, .raw = split, .ldraw = 2 * l.cin}));
    } else {
        CKP(h.h);
        CK(r.gn({h.h, c1, false}, HW, p + ".in_layers.0", 1e-5f, 1, t, {.x2 = skip ? skip->h : nullptr, .C2 = skip_c}));
    }
    const int off = e->emb_off[p];
    void* h1 = h1f ? (void*)e->f32("rb.h1f", (size_t)M * l.cout) : (void*)e->h16("rb.h1", (size_t)M * l.cout);
    CKP(h1);
    const void* emb = precise ? (const void*)(reinterpret_cast<const float*>(emb_out) + off) : (const void*)(reinterpret_cast<const half_t*>(emb_out) + off);
    CK(r.conv({t, strict ? 2 * l.cin : l.cin, strict}, p + ".in_layers.2", Bn, sh, sw, h1, h1f ? GL_OUT_F32_ROWMAJOR : GL_OUT_F16_ROWMAJOR,
              {.epi = GL_EPI_ROWBIAS, .rowbias = {emb, e->emb_total, HW}}));
    CK(r.gn({h1, l.cout, h1f}, HW, p + ".out_layers.0", 1e-5f, 1, t2, {.ldo = strict ? 2 * l.cout : 0, .out_lo = strict ? t2 + l.cout : nullptr}));
    const float* sk = h.f;
    if (has_skip_conv) {
        float* skb = e->f32("rb.skip.f32", (size_t)M * l.cout);
        CKP(skb);
        if (precise) {
            CK(r.gemm({split, 2 * l.cin, true}, p + ".skip_connection", M, skb, l.cout, {.out_mode = GL_OUT_F32_ROWMAJOR, .wsplit = true}));
        } else {                // th.cat([h, skip]) folded in: the K columns from c1 on read the skip tensor
            CK(r.gemm({h.h, c1}, p + ".skip_connection", M, skb, l.cout,
                      {.out_mode = GL_OUT_F32_ROWMAJOR, .a2 = {skip ? skip->h : nullptr, skip_c}, .ksplit = skip ? c1 : 0, .wsplit = true}));
        }
        sk = skb;
    } else if (skip) {
        return GL_ERR_BAD_ARG;
    }
    out->f = e->f32(tag + ".f32", (size_t)M * l.cout);
    out->h = need_h ? e->h16(tag, (size_t)M * l.cout) : nullptr;
    CKP(out->f);
    if (need_h) CKP(out->h);
    return r.conv({t2, strict ? 2 * l.cout : l.cout, strict}, p + ".out_layers.3", Bn, sh, sw, out->f, GL_OUT_F32_ROWMAJOR,
                  {.epi = GL_EPI_RES, .res = {sk, l.cout, true}, .out2 = out->h});
}

// SpatialTransformer.forward + BasicTransformerBlock._forward (attention.py:436-446, :394-402)
// share_half: xin holds only the first Bn / 2 samples (the shared cond / uncond prefix): GroupNorm .. attn1 run on those rows, then xin and x
// are duplicated into the second half and the block continues on all Bn samples (from the first conditioning-dependent op on).
int spatial_transformer(Run& r, const LayerD& l, int li, Stream2 xin, int sh, int sw, bool fuser_on, const std::string& tag, bool need_h, Stream2* out,
                        bool share_half = false) {
    gl_engine* e = r.e;
    const gl_unet_config& cfg = e->cfg;
    const std::string& p = l.prefix;
    const std::string t = p + ".transformer_blocks.0";
    const int C = l.cin, d = l.d_head, H = cfg.num_heads;
    const int Bn = e->Bn, N = sh * sw, M = Bn * N, mo = cfg.max_objs, ng = n_ground(cfg), R = e->R, Lc = e->Lc;
    const std::string sl = std::to_string(li);
    float* xa = e->f32("st.xa", (size_t)M * C);
    float* xb = e->f32("st.xb", (size_t)M * C);
    const bool strict = g_strict != 0;
    const bool precise = g_precise != 0 || strict;
    const int lnw = strict ? 2 * C : C;          // strict: every LayerNorm writes [hi | lo] rows for the projection behind it
    half_t* g0 = e->h16("st.gn", (size_t)M * C * (precise ? 2 : 1));
    half_t* lnb = e->h16("st.ln", (size_t)M * lnw);
    CKP(xa); CKP(xb); CKP(g0); CKP(lnb);
    const float* gates = e->f32("gates", e->st_layers.size() * 4) + (size_t)li * 4;
    float* x = xa;
    auto nxt = [&](float* cur) { return cur == xa ? xb : xa; };
    {
        const int B1 = share_half ? Bn / 2 : Bn, M1 = B1 * N;
        BnScope half(e, B1);              // self_attention reads e->Bn
        if (precise) {
            // Normalize on the fp32 stream, rows written as [hi | lo]; proj_in takes both halves against the same weight
            CK(r.gn({xin.f, C, true}, N, p + ".norm", 1e-6f, 0, g0, {.ldo = 2 * C, .out_lo = g0 + C}));
            CK(r.gemm({g0, 2 * C, true}, p + ".proj_in", M1, x, C, {.out_mode = GL_OUT_F32_ROWMAJOR, .wsplit = true}));
        } else {
            CKP(xin.h);
            CK(r.gn({xin.h, C, false}, N, p + ".norm", 1e-6f, 0, g0));
            CK(r.gemm({g0, C}, p + ".proj_in", M1, x, C, {.out_mode = GL_OUT_F32_ROWMAJOR, .wsplit = true}));
        }
        // --- attn1 (attention.py:395)
        half_t* att1 = nullptr;
        CK(r.ln({x, C, true}, lnb, lnw, t + ".norm1", N, C, {.y_lo = strict}));
        CK(self_attention(r, lnb, N, N, N, C, d, t + ".attn1", "st.sa", &att1));
        float* y = nxt(x);
        CK(r.gemm({att1, lnw, strict}, t + ".attn1.o", M1, y, C, {.out_mode = GL_OUT_F32_ROWMAJOR, .epi = GL_EPI_RES, .res = {x, C, true}}));
        x = y;
        if (share_half) {
            // the uncond half: identical up to here (same latent, t, weights; attention.py:395 is the last op before the conditioning enters)
            CK(r.dup_rows(x, (size_t)M1 * C * 4));
            CK(r.dup_rows(xin.f, (size_t)M1 * C * 4));
            if (xin.h) CK(r.dup_rows(xin.h, (size_t)M1 * C * 2));
        }
    }
    half_t* att = nullptr;
    // --- gated self-attention fuser over [x ; objs] (attention.py:226-234); exact identity at scale 0
    if (fuser_on) {
        const std::string f = t + ".fuser";
        // [x ; objs] rows per sample padded to a multiple of 8 so that the QKV epilogue can store V^T in 16-byte pieces; the
        // pad rows are never normalised into (arbitrary finite-or-not contents): as keys they are masked by the attention
        // kernel (Nk = N + ng), as queries they are not used (Nq = N).  ng = the grounding-token count (n_ground): max_objs, or
        // 2 * max_objs on a text_image handle, up to 136 (17 per person) on a keypoint handle; the relation chain below keeps
        // mo = max_objs boxes
        const int rows = N + ((ng + 7) & ~7);
        half_t* cat = e->h16("st.cat", (size_t)Bn * rows * lnw);
        CKP(cat);
        // the hoisted fuser.linear(objs): fp32 from split-fp16 operands (strict), fp32 (precise) or fp16 rows
        const void* objs = strict    ? (const void*)e->f32("hoist.objs32s." + sl, (size_t)Bn * ng * C)
                           : precise ? (const void*)e->f32("hoist.objs32." + sl, (size_t)Bn * ng * C)
                                     : (const void*)e->h16("hoist.objs." + sl, (size_t)Bn * ng * C);
        CK(r.ln({x, C, true}, cat, lnw, f + ".norm1", N, C, {.rows_out = rows, .x2 = {objs, C, precise}, .rows2 = ng, .y_lo = strict}));
        CK(self_attention(r, cat, rows, N, N + ng, C, d, f + ".attn", "st.fa", &att));
        float* y = nxt(x);
        CK(r.gemm({att, lnw, strict}, f + ".attn.o", M, y, C, {.out_mode = GL_OUT_F32_ROWMAJOR, .epi = GL_EPI_GATE_RES, .res = {x, C, true}, .gate = gates + 0}));
        x = y;
        CK(r.ln({x, C, true}, lnb, lnw, f + ".norm2", N, C, {.y_lo = strict}));
        y = nxt(x);
        CK(feed_forward(r, lnb, x, f + ".ff", M, C, y, GL_OUT_F32_ROWMAJOR, gates + 1));
        x = y;
    }
    // --- relation injection (attention.py:315-359, :398), closed form
    // (a no_relation handle has no such chain: the fuser's output -- attn1's at fuser scale 0 -- goes straight to LayerNorm(norm2) -> attn2,
    // attention_original.py:312-316)
    bool ln2_done = false;
    if (!cfg.no_relation) {
        const std::string rf = t + ".rela_fuse";
        const std::string ss = level_tag(sh, sw);
        const int* rects = reinterpret_cast<const int*>(e->buf("cond.rects." + ss, (size_t)Bn * mo * 16));
        const int* nvalid = reinterpret_cast<const int*>(e->buf("cond.nvalid." + ss, (size_t)Bn * 4));
        const int* poison = reinterpret_cast<const int*>(e->buf("cond.poison." + ss, (size_t)Bn * 4));
        const int ms = e->rel_slots > 0 ? e->rel_slots : mo;      // rows per sample of the chain (feat .. f2); rects keep max_objs slots
        const int Mo = Bn * ms;
        float* stats = e->f32("st.lnstats", (size_t)M * 2);
        half_t* hid = e->h16("st.hid", (size_t)M * C);
        half_t* feat = e->h16("rl.feat", (size_t)Mo * C);
        half_t* fn = e->h16("rl.ln", (size_t)Mo * C);
        half_t* q = e->h16("rl.q", (size_t)Mo * C);
        half_t* ar = e->h16("rl.att", (size_t)Mo * C);
        half_t* f1 = e->h16("rl.f1", (size_t)Mo * C);
        half_t* hg = e->h16("rl.ffh", (size_t)Mo * 4 * C);
        half_t* f2 = e->h16("rl.f2", (size_t)Mo * C);
        CKP(rects); CKP(nvalid); CKP(poison); CKP(stats); CKP(hid); CKP(feat); CKP(fn); CKP(q); CKP(ar); CKP(f1); CKP(hg); CKP(f2);
        if (precise) {
            // LayerNorm3 is never materialised: its per-row statistics, then the box means of LN3(x) and (in rela_merge) LN3(x) itself in fp32
            r.launches += 2;
            CK(gl_layernorm_stats(x, C, M, C, 1e-5f, stats, r.st));
            CK(gl_rela_pool_ln3(x, stats, e->Wf(rf + ".norm3.g"), e->Wf(rf + ".norm3.b"), Bn, sh, sw, C, rects, nvalid, poison, mo, ms, feat,
                                e->Wf(rf + ".norm1.g"), e->Wf(rf + ".norm1.b"), fn, r.st));
        } else {
            CK(r.ln({x, C, true}, hid, C, rf + ".norm3", N, C, {.stats = stats}));
            ++r.launches;
            CK(gl_rela_pool(hid, Bn, sh, sw, C, rects, nvalid, poison, mo, ms, feat, e->Wf(rf + ".norm1.g"), e->Wf(rf + ".norm1.b"), fn, r.st));
        }
        CK(r.gemm({fn, C}, rf + ".attn.q", Mo, q, C, {.bias = false}));
        const half_t* kv = e->h16("hoist.kvrel." + sl, (size_t)Bn * R * 2 * C);
        const int ldvt = vt_ld(R);
        const half_t* vtr = e->h16("hoist.vtrel." + sl, (size_t)Bn * H * d * ldvt);
        CKP(kv); CKP(vtr);
        CK(r.attn({q, (int64_t)ms * C, C}, {kv, (int64_t)R * 2 * C, 2 * C}, {vtr, ldvt}, {ar, (int64_t)ms * C, C}, d, ms, R));
        CK(r.gemm({ar, C}, rf + ".attn.o", Mo, f1, C, {.epi = GL_EPI_GATE_RES, .res = {feat, C, false}, .gate = gates + 2}));
        CK(r.ln({f1, C, false}, fn, C, rf + ".norm2", ms, C));
        CK(r.gemm({fn, C}, rf + ".ff.ff1", Mo, hg, 4 * C, {.epi = GL_EPI_GEGLU}));
        CK(r.gemm({hg, 4 * C}, rf + ".ff.ff2", Mo, f2, C, {.epi = GL_EPI_GATE_RES, .res = {f1, C, false}, .gate = gates + 3}));
        float* y = nxt(x);
        ++r.launches;
        // ... and LayerNorm(norm2) of the merged rows in the same launch (the rows attn2's q projection reads)
        const bool fuse_ln2 = g_fuse_merge_ln && ms <= 32 && !strict;      // (strict: norm2 is a launch of its own that also writes the lo half)
        CK(gl_rela_merge(x, 1, nullptr, stats, e->Wf(rf + ".norm3.g"), e->Wf(rf + ".norm3.b"), f2, Bn, sh, sw, C, rects, nvalid, poison, mo, ms, y,
                         fuse_ln2 ? e->Wf(t + ".norm2.g") : nullptr, fuse_ln2 ? e->Wf(t + ".norm2.b") : nullptr, fuse_ln2 ? lnb : nullptr, r.st));
        x = y;
        ln2_done = fuse_ln2;
    }
    // --- attn2: text cross-attention with hoisted K/V (attention.py:400)
    {
        half_t* q2 = e->h16("st.q2", (size_t)M * lnw);
        half_t* a2 = e->h16("st.att2", (size_t)M * lnw);
        const int ldvt = vt_ld(Lc);
        CKP(q2); CKP(a2);
        float* y = nxt(x);
        if (strict) {
            // hoisted K / V of the text context as [k v | k_lo v_lo] rows and V^T hi / lo (gl_set_conditioning, split_weights handles)
            const half_t* kv = e->h16("hoist.kvctxs." + sl, (size_t)Bn * Lc * 4 * C);
            const half_t* vtc = e->h16("hoist.vtctxs." + sl, (size_t)2 * Bn * H * d * ldvt);
            CKP(kv); CKP(vtc);
            CK(r.ln({x, C, true}, lnb, lnw, t + ".norm2", N, C, {.y_lo = true}));
            CK(r.gemm({lnb, lnw, true}, t + ".attn2.q", M, q2, lnw, {.bias = false, .out_mode = GL_OUT_F16_HILO}));
            CK(r.attn({q2, (int64_t)N * lnw, lnw, q2 + C}, {kv, (int64_t)Lc * 4 * C, 4 * C, kv + 2 * C}, {vtc, ldvt, vtc + (size_t)Bn * H * d * ldvt},
                      {a2, (int64_t)N * lnw, lnw, a2 + C}, d, N, Lc));
            CK(r.gemm({a2, lnw, true}, t + ".attn2.o", M, y, C, {.out_mode = GL_OUT_F32_ROWMAJOR, .epi = GL_EPI_RES, .res = {x, C, true}}));
        } else {
            const half_t* kv = e->h16("hoist.kvctx." + sl, (size_t)Bn * Lc * 2 * C);
            const half_t* vtc = e->h16("hoist.vtctx." + sl, (size_t)Bn * H * d * ldvt);
            CKP(kv); CKP(vtc);
            if (!ln2_done) CK(r.ln({x, C, true}, lnb, C, t + ".norm2", N, C));
            CK(r.gemm({lnb, C}, t + ".attn2.q", M, q2, C, {.bias = false}));
            CK(r.attn({q2, (int64_t)N * C, C}, {kv, (int64_t)Lc * 2 * C, 2 * C}, {vtc, ldvt}, {a2, (int64_t)N * C, C}, d, N, Lc));
            CK(r.gemm({a2, C}, t + ".attn2.o", M, y, C, {.out_mode = GL_OUT_F32_ROWMAJOR, .epi = GL_EPI_RES, .res = {x, C, true}}));
        }
        x = y;
    }
    // --- GEGLU feed-forward (attention.py:401): the sum is only consumed by proj_out's matrix product -> fp16
    // (precise: as [hi | lo] rows, proj_out takes both halves against the same weight)
    half_t* x16 = e->h16("st.x6", (size_t)M * C * (precise ? 2 : 1));
    CKP(x16);
    CK(r.ln({x, C, true}, lnb, lnw, t + ".norm3", N, C, {.y_lo = strict}));
    CK(feed_forward(r, lnb, x, t + ".ff", M, C, x16, precise ? GL_OUT_F16_HILO : GL_OUT_F16_ROWMAJOR, nullptr));
    // --- proj_out + residual (attention.py:444-446)
    out->f = e->f32(tag + ".f32", (size_t)M * C);
    out->h = need_h ? e->h16(tag, (size_t)M * C) : nullptr;
    CKP(out->f);
    if (need_h) CKP(out->h);
    return r.gemm({x16, precise ? 2 * C : C, precise}, p + ".proj_out", M, out->f, C,
                  {.out_mode = GL_OUT_F32_ROWMAJOR, .epi = GL_EPI_RES, .res = {xin.f, C, true}, .out2 = out->h, .ldc2 = C, .wsplit = true});
}

int launch_forward(gl_engine* e, int reps, bool fuser_on, bool sd_conv, bool uniform_t, hipStream_t st, int* n_launches) {
    const gl_unet_config& cfg = e->cfg;
    const int Bn = e->Bn, mc = cfg.model_channels;
    // [cond ; uncond] batch over ONE set of latents and one timestep: the two halves are identical until the first op that reads the
    // conditioning (fuser / rela_fuse / attn2 of the first transformer block) -- run that prefix once on Bn / 2 samples
    const bool share = g_share != 0 && reps == 2 && uniform_t && (Bn % 2) == 0 && e->input_blocks.size() > 1 &&
                       !e->input_blocks[1].layers.empty() && e->input_blocks[1].layers[0].kind == RES;
    const int B0 = share ? Bn / 2 : Bn;
    int sh = e->lat_h, sw = e->lat_w;
    Run r{e, st, e->buf("splitk.ws", GL_WS_BYTES)};
    CKP(r.ws);
    const float* x_lat = e->f32("in.xlat", (size_t)(Bn / reps) * cfg.in_channels * sh * sw);
    const float* t_buf = e->f32("in.t", Bn);
    float* eps = e->f32("out.eps", (size_t)Bn * cfg.out_channels * sh * sw);
    CKP(x_lat); CKP(t_buf); CKP(eps);
    // time embedding (openaimodel.py:428-429) and all emb_layers in one GEMM (:172-178, :220)
    const bool strict = g_strict != 0;
    if (strict && !e->cfg.split_weights) { e->err = "strict mode (option 50) needs a handle created with split_weights"; return GL_ERR_BAD_ARG; }
    const bool precise = g_precise != 0 || strict;
    const int tw = strict ? 2 : 1;                 // strict: the time-embedding rows are [hi | lo] all the way
    half_t* te = e->h16("te.sin", (size_t)Bn * mc * tw);
    half_t* e1 = e->h16("te.e1", (size_t)Bn * 4 * mc * tw);
    half_t* e2 = e->h16("te.e2", (size_t)Bn * 4 * mc * tw);
    // (precise mode: the 22 emb_layers outputs stay fp32 -- they are added to every element of a ResBlock's first conv result)
    void* emb_out = precise ? (void*)e->f32("te.out32", (size_t)Bn * e->emb_total) : (void*)e->h16("te.out", (size_t)Bn * e->emb_total);
    CKP(te); CKP(e1); CKP(e2); CKP(emb_out);
    ++r.launches;
    if (strict) {
        float* te32 = e->f32("te.sin32", (size_t)Bn * mc);
        CKP(te32);
        CK(gl_timestep_embedding_f32(t_buf, Bn, mc, te32, st));
        CK(r.split(te32, Bn, mc, te));
    } else {
        CK(gl_timestep_embedding(t_buf, Bn, mc, te, st));
    }
    const int tom = strict ? GL_OUT_F16_HILO : GL_OUT_F16_ROWMAJOR;
    CK(r.gemm({te, mc * tw, strict}, "time_embed.0", Bn, e1, 4 * mc * tw, {.out_mode = tom, .epi = GL_EPI_SILU}));
    CK(r.gemm({e1, 4 * mc * tw, strict}, "time_embed.2", Bn, e2, 4 * mc * tw, {.out_mode = tom, .epi = GL_EPI_SILU}));
    CK(r.gemm({e2, 4 * mc * tw, strict}, "emb_all", Bn, emb_out, e->emb_total, {.out_mode = precise ? GL_OUT_F32_ROWMAJOR : GL_OUT_F16_ROWMAJOR}));
    // first conv on the zero-padded NHWC latent (openaimodel.py:299, :393-405)
    half_t* xin = e->h16("in.x", (size_t)Bn * sh * sw * CIN_PAD);
    CKP(xin);
    ++r.launches;
    const int n_extra = extra_channels(cfg, e->ground_extra);
    if (n_extra != 0 && !sd_conv) {
        // cat([x, inpainting_extra_input], dim=1) (openaimodel.py:439) folded into the pack: one launch, like the text handle's.  Both CFG halves
        // read the same extra (plms.py:118-121), so the shared prefix stays valid.  A spatial handle's downsampled grounding_extra_input goes the
        // same way while the GLIGEN conv is in place; its SD-conv variant reads the latent alone.
        const float* extra = e->f32("in.extra", (size_t)e->extra_bs * n_extra * sh * sw);
        CKP(extra);
        CK(gl_pack_latent_extra(x_lat, extra, Bn / reps, e->extra_bs, cfg.in_channels, n_extra, sh * sw, CIN_PAD, share ? 1 : reps,
                                g_in_split && 3 * first_conv_in(cfg, e->ground_extra) <= CIN_PAD, xin, st));
    } else {
        CK(gl_pack_latent(x_lat, Bn / reps, cfg.in_channels, sh * sw, CIN_PAD, share ? 1 : reps, g_in_split && 3 * cfg.in_channels <= CIN_PAD, xin, st));
    }
    // fp16 copies of stream tensors: only where a down / up conv consumes the tensor (precise mode: every GroupNorm and 1x1 conv
    // reads the fp32 stream), or everywhere in the round-3 fp16-copy mode
    auto first_kind = [&](const BlockD* b) { return b && !b->layers.empty() ? b->layers[0].kind : -1; };
    auto wants_h = [&](int next_kind) { return !precise || next_kind == DOWN || next_kind == UP; };
    Stream2 h;
    h.f = e->f32("skip.0.f32", (size_t)Bn * sh * sw * mc);
    h.h = wants_h(first_kind(e->input_blocks.size() > 1 ? &e->input_blocks[1] : nullptr)) ? e->h16("skip.0", (size_t)Bn * sh * sw * mc) : nullptr;
    CKP(h.f);
    CK(r.conv({xin, CIN_PAD}, sd_conv ? "sd_first_conv" : "input_blocks.0.0", B0, sh, sw, h.f, GL_OUT_F32_ROWMAJOR, {.out2 = h.h}));
    if (share) {            // skip-stack entry 0 is consumed at full batch by the last output block
        CK(r.dup_rows(h.f, (size_t)B0 * sh * sw * mc * 4));
        if (h.h) CK(r.dup_rows(h.h, (size_t)B0 * sh * sw * mc * 2));
    }
    struct Skip { Stream2 s; int h, w, c; };
    std::vector<Skip> skips{{h, sh, sw, mc}};
    int st_idx = 0;
    int h_c = mc;

    auto run_block = [&](const BlockD& b, const std::string& bi, const Skip* skip, const BlockD* next, bool half_first = false) -> int {
        const Stream2* sk = skip ? &skip->s : nullptr;
        int sk_c = skip ? skip->c : 0;
        bool half_pending = false;          // h holds only the first Bn / 2 samples (shared prefix)
        for (size_t j = 0; j < b.layers.size(); ++j) {
            const LayerD& l = b.layers[j];
            const std::string tag = bi + "." + std::to_string(j);
            const bool need_h = wants_h(j + 1 < b.layers.size() ? b.layers[j + 1].kind : first_kind(next));
            Stream2 o;
            if (l.kind == RES) {
                if (half_first && j == 0) {
                    // the block's output tensors at FULL size first (the pool hands back the same buffers to the half-batch call below)
                    CKP(e->f32(tag + ".f32", (size_t)Bn * sh * sw * l.cout));
                    if (need_h) CKP(e->h16(tag, (size_t)Bn * sh * sw * l.cout));
                    BnScope half(e, B0);
                    CK(res_block(r, l, h, sk, sk_c, sh, sw, emb_out, tag, need_h, &o));
                    half_pending = true;
                } else {
                    CK(res_block(r, l, h, sk, sk_c, sh, sw, emb_out, tag, need_h, &o));
                }
                sk = nullptr; sk_c = 0;
            } else if (l.kind == ST) {
                CK(spatial_transformer(r, l, st_idx++, h, sh, sw, fuser_on, tag, need_h, &o, half_pending));
                half_pending = false;       // the transformer duplicated its input and its own stream after attn1
            } else if (l.kind == DOWN || l.kind == UP) {
                const bool up = l.kind == UP;
                const int oh = up ? sh * 2 : sh / 2, ow = up ? sw * 2 : sw / 2;
                o.f = e->f32(tag + ".f32", (size_t)Bn * oh * ow * l.cout);
                o.h = need_h ? e->h16(tag, (size_t)Bn * oh * ow * l.cout) : nullptr;
                CKP(o.f); CKP(h.h);
                if (need_h) CKP(o.h);
                Run::Act in{h.h, l.cin};
                if (strict) {          // the stream tensor itself as [hi | lo] pixel rows
                    half_t* hs = e->h16("conv.split", (size_t)Bn * sh * sw * 2 * l.cin);
                    CKP(hs);
                    CK(r.split(h.f, (int64_t)Bn * sh * sw, l.cin, hs));
                    in = {hs, 2 * l.cin, true};
                }
                CK(r.conv(in, l.prefix, Bn, sh, sw, o.f, GL_OUT_F32_ROWMAJOR, {.stride = up ? 1 : 2, .ups = up, .out2 = o.h}));
                sh = oh; sw = ow;
            } else {
                return GL_ERR_BAD_ARG;
            }
            h = o;
            h_c = l.cout;
            if (half_pending && !(j + 1 < b.layers.size() && b.layers[j + 1].kind == ST)) {
                CK(r.dup_rows(h.f, (size_t)B0 * sh * sw * h_c * 4));
                if (h.h) CK(r.dup_rows(h.h, (size_t)B0 * sh * sw * h_c * 2));
                half_pending = false;
            }
        }
        return 0;
    };

    for (size_t i = 1; i < e->input_blocks.size(); ++i) {
        CK(run_block(e->input_blocks[i], "skip." + std::to_string(i), nullptr, i + 1 < e->input_blocks.size() ? &e->input_blocks[i + 1] : &e->middle,
                     share && i == 1));
        skips.push_back({h, sh, sw, h_c});
    }
    CK(run_block(e->middle, "mid", nullptr, e->output_blocks.empty() ? nullptr : &e->output_blocks[0]));
    for (size_t i = 0; i < e->output_blocks.size(); ++i) {
        const Skip sk = skips.back();
        skips.pop_back();
        if (sk.h != sh || sk.w != sw) return GL_ERR_BAD_ARG;
        CK(run_block(e->output_blocks[i], "out." + std::to_string(i), &sk, i + 1 < e->output_blocks.size() ? &e->output_blocks[i + 1] : nullptr));
    }
    const int ocl = e->out_channels_last;
    half_t* g = e->h16("fin.gn", (size_t)Bn * sh * sw * ocl * (strict ? 2 : 1));
    CKP(g);
    if (!precise) CKP(h.h);
    CK(r.gn({precise ? (const void*)h.f : (const void*)h.h, ocl, precise}, sh * sw, "out.0", 1e-5f, 1, g,
            {.ldo = strict ? 2 * ocl : 0, .out_lo = strict ? g + ocl : nullptr}));
    CK(r.conv({g, strict ? 2 * ocl : ocl, strict}, "out.2", Bn, sh, sw, eps, GL_OUT_F32_NCHW, {.nchw_hw = sh * sw}));
    if (n_launches) *n_launches = r.launches;
    return 0;
}

}  // namespace

// ====================================================================================== C ABI
extern "C" int gl_create(const gl_unet_config* cfg, gl_engine** out) {
    if (!cfg || !out) return GL_ERR_BAD_ARG;
    if (cfg->n_levels <= 0 || cfg->n_levels > 8 || cfg->n_attn_res < 0 || cfg->n_attn_res > 8 || cfg->num_heads <= 0) return GL_ERR_BAD_ARG;
    if (cfg->model_channels % 64 || cfg->context_dim % 64 || cfg->pos_in_dim % 8 || cfg->pos_out_dim != cfg->context_dim) return GL_ERR_UNSUPPORTED;
    if (cfg->grounding < 0 || (cfg->grounding > 2 && cfg->grounding != 4) || cfg->max_objs <= 0) return GL_ERR_UNSUPPORTED;
    if (cfg->grounding == 2) {
        // keypoint: 17 tokens per person, at most 8 persons; the first MLP layer's K is padded (pin_width), so no % 64 rule on it; no relation
        // chain (it pools over boxes) and no inpainting (its mask is drawn from boxes)
        if (cfg->no_relation != 1 || cfg->inpaint_mode != 0 || (cfg->max_objs % 17) != 0 || cfg->max_objs > 136) return GL_ERR_UNSUPPORTED;
        if (cfg->pos_in_dim != cfg->pos_out_dim) return GL_ERR_UNSUPPORTED;
    } else if (cfg->grounding == 4) {
        // spatial: finished tokens come in (no PositionNet in the table, so no rule on pos_in_dim + Fourier width); the upstream block only, no
        // inpainting, no split-fp16 table (the tokenizer has no strict form); max_objs counts tokens, the gated self-attention's 64 at most
        if (cfg->no_relation != 1 || cfg->inpaint_mode != 0 || cfg->split_weights != 0 || cfg->max_objs > 64) return GL_ERR_UNSUPPORTED;
    } else {
        if ((cfg->pos_in_dim + 8 * cfg->fourier_freqs) % 64) return GL_ERR_UNSUPPORTED;
        if (n_ground(*cfg) > 64) return GL_ERR_UNSUPPORTED;
    }
    if (cfg->no_relation != 0 && cfg->no_relation != 1) return GL_ERR_UNSUPPORTED;
    if ((cfg->inpaint_mode != 0 && cfg->inpaint_mode != 1) || first_conv_in(*cfg) > CIN_PAD) return GL_ERR_UNSUPPORTED;
    gl_engine* e = new gl_engine();
    e->cfg = *cfg;
    e->fold_up = gl_opt(55) == 1 && !cfg->split_weights;      // read ONCE: the table (and every rank's layout built from it) follows
    build_plan(e);
    build_table(e);
    *out = e;
    return 0;
}

extern "C" int gl_destroy(gl_engine* e) {
    if (!e) return GL_ERR_BAD_ARG;
    e->cache.release();
    e->pool.release();
    for (int k = 0; k < 2; ++k) {
        if (e->gate_pin_ev[k]) { (void)hipEventSynchronize(e->gate_pin_ev[k]); (void)hipEventDestroy(e->gate_pin_ev[k]); }
        if (e->gate_pin[k]) (void)hipHostFree(e->gate_pin[k]);
    }
    delete e;
    return 0;
}

extern "C" int gl_num_weights(const gl_engine* e) { return e ? (int)e->wt.names.size() : GL_ERR_BAD_ARG; }
extern "C" int64_t gl_weights_bytes(const gl_engine* e) { return e ? e->wt.total : -1; }
extern "C" int gl_weight_at(const gl_engine* e, int32_t i, gl_weight_info* info) { return e ? e->wt.info_at(i, info) : GL_ERR_BAD_ARG; }

extern "C" int gl_load_weights(gl_engine* e, const void* packed, int64_t bytes, int32_t has_sd_conv, void* stream) {
    if (!e || !packed || bytes < e->wt.total) return GL_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(packed) % 16) return GL_ERR_BAD_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return GL_ERR_BAD_ARG;
    e->device = dev;
    CK(gl_init());
    e->wt.wbase = reinterpret_cast<const char*>(packed);
    if (has_sd_conv && e->cfg.inpaint_mode) {
        e->err = "gl_load_weights: an inpaint_mode handle has no sd_first_conv slots (its first conv is not restorable)";
        return GL_ERR_BAD_ARG;
    }
    e->has_sd = has_sd_conv != 0;
    e->cache.drop();
    // the scalar gates tanh(alpha) live in the packed buffer; fetch them once (tiny, synchronous)
    const size_t n = e->st_layers.size();
    e->gate_tanh.assign(n * 4, 0.0f);
    hipStream_t st = (hipStream_t)stream;
    if (hipStreamSynchronize(st) != hipSuccess) return GL_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i) {
        const std::string t = e->st_layers[i].prefix + ".transformer_blocks.0";
        const char* names[4] = {".fuser.tanh_attn", ".fuser.tanh_dense", ".rela_fuse.tanh_attn", ".rela_fuse.tanh_dense"};
        for (int k = 0; k < (e->cfg.no_relation ? 2 : 4); ++k)     // (no_relation: slots 2 and 3 keep their place, unused)
            if (hipMemcpy(&e->gate_tanh[i * 4 + k], e->W(t + names[k]), sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return GL_ERR_BAD_ARG;
    }
    e->fuser_scale_cur = -1e30f;
    return 0;
}

// ---- the grounding family of a handle (gl_unet_config.grounding), everything the conditioning code asks of it, in one place:
//   GroundIn      the grounding tensors a conditioning entry takes.  loc: boxes [Bn, mo, 4], or points [Bn, mo, 2] on a keypoint handle; emb: the
//                 phrase embeddings (positive_embeddings of the text PositionNet, text_embeddings of the text_image one); text_masks / image_masks
//                 / image_emb: the three further inputs of a text_image handle.  What a family does not take stays NULL
//   kept_inputs   those of them the family reads, with the pool tags a split_weights handle keeps device copies under for the lazy strict hoists
//   posnet_input  the kernel that builds the MLP input rows of every chain ([nch, Bn * mo] chain-major rows of pin_width columns)
//   posnet_chains / posnet_chain   the MLP chains those rows feed
//                 tokens: the finished grounding tokens [Bn, mo, D] of a spatial handle, which has no PositionNet of its own
struct GroundIn {
    const float *loc = nullptr, *masks = nullptr, *emb = nullptr, *text_masks = nullptr, *image_masks = nullptr, *image_emb = nullptr, *tokens = nullptr;
};
struct KeptIn { const char* tag; const float* GroundIn::*field; size_t n; };

static std::vector<KeptIn> kept_inputs(const gl_unet_config& c, int Bn) {
    const size_t rows = (size_t)Bn * c.max_objs;
    if (c.grounding == 4) return {{"cond.in.tokens", &GroundIn::tokens, rows * c.pos_out_dim}};
    if (c.grounding == 2) return {{"cond.in.points", &GroundIn::loc, rows * 2}, {"cond.in.masks", &GroundIn::masks, rows}};
    std::vector<KeptIn> k{{"cond.in.boxes", &GroundIn::loc, rows * 4}, {"cond.in.masks", &GroundIn::masks, rows}, {"cond.in.posemb", &GroundIn::emb, rows * c.pos_in_dim}};
    if (c.grounding == 1) {
        k.push_back({"cond.in.tmasks", &GroundIn::text_masks, rows});
        k.push_back({"cond.in.imasks", &GroundIn::image_masks, rows});
        k.push_back({"cond.in.imgemb", &GroundIn::image_emb, rows * c.pos_in_dim});
    }
    return k;
}
static int posnet_chains(const gl_unet_config& c) { return c.grounding == 1 ? 2 : 1; }      // text (+ image); one for text and for keypoint
static const char* posnet_chain(const gl_unet_config& c, int chain) {
    return c.grounding != 1 ? "position_net.linears" : (chain == 0 ? "position_net.linears_text" : "position_net.linears_image");
}
// out: fp16 rows, or fp32 rows with f32 (the strict chain, split into [hi | lo] afterwards)
static int posnet_input(gl_engine* e, const GroundIn& in, int Bn, bool f32, void* out, hipStream_t st) {
    const gl_unet_config& c = e->cfg;
    const int rows = Bn * c.max_objs, F = c.fourier_freqs;
    float* o32 = reinterpret_cast<float*>(out);
    if (c.grounding == 2) {
        const float *pe = e->Wf("position_net.person_emb"), *ke = e->Wf("position_net.keypoint_emb"), *np = e->Wf("position_net.null_person"),
                    *nx = e->Wf("position_net.null_xy");
        return f32 ? gl_posnet_input_kp_f32(in.loc, in.masks, pe, ke, np, nx, Bn, c.max_objs, c.pos_in_dim, F, o32, st)
                   : gl_posnet_input_kp(in.loc, in.masks, pe, ke, np, nx, Bn, c.max_objs, c.pos_in_dim, F, out, st);
    }
    if (c.grounding == 1) {
        const float *nt = e->Wf("position_net.null_text"), *ni = e->Wf("position_net.null_image"), *nx = e->Wf("position_net.null_xyxy");
        const size_t o = (size_t)rows * pin_width(c);            // the image chain's rows follow the text chain's
        return f32 ? gl_posnet_input_ti_f32(in.loc, in.masks, in.text_masks, in.image_masks, in.emb, in.image_emb, nt, ni, nx, rows, c.pos_in_dim, F, o32,
                                            o32 + o, st)
                   : gl_posnet_input_ti(in.loc, in.masks, in.text_masks, in.image_masks, in.emb, in.image_emb, nt, ni, nx, rows, c.pos_in_dim, F, out,
                                        reinterpret_cast<half_t*>(out) + o, st);
    }
    const float *np = e->Wf("position_net.null_pos"), *nx = e->Wf("position_net.null_xyxy");
    return f32 ? gl_posnet_input_f32(in.loc, in.masks, in.emb, np, nx, rows, c.pos_in_dim, F, o32, st)
               : gl_posnet_input(in.loc, in.masks, in.emb, np, nx, rows, c.pos_in_dim, F, out, st);
}

// Strict mode's hoists (handles created with split_weights): the conditioning tensors from split-fp16 operands all the way -- PositionNet on fp32
// inputs split into [hi | lo], every Linear with [hi | lo] activations (+ the third pass x.Wlo, key 51), K / V of the text context as
// [k v | k_lo v_lo] rows with V^T hi / lo, fuser.linear(objs) in fp32.  Computed LAZILY: gl_set_conditioning keeps device copies of
// its inputs on such a handle and runs this only when option 50 is set at that time; otherwise the first strict forward does (outside any
// capture), and again when key 51 changed since -- a split handle that stays in default mode never pays for the chain.
int strict_hoists(gl_engine* e, hipStream_t st) {
    const gl_unet_config& cfg = e->cfg;
    const int Bn = e->Bn, Lc = e->Lc, mo = cfg.max_objs, ng = n_ground(cfg), ctx = cfg.context_dim, H = cfg.num_heads;
    const bool ti = cfg.grounding == 1;
    const int nch = posnet_chains(cfg);
    const int pin_dim = pin_width(cfg);
    const float* context = e->f32("cond.in.context", (size_t)Bn * Lc * ctx);
    CKP(context);
    GroundIn in;                                     // the device copies set_conditioning kept
    for (const KeptIn& k : kept_inputs(cfg, Bn)) {
        in.*(k.field) = e->f32(k.tag, k.n);
        CKP(in.*(k.field));
    }
    Run r{e, st, e->buf("splitk.ws", GL_WS_BYTES)};
    CKP(r.ws);
    gl_opts strict_opts = *(tl_gl_opts ? tl_gl_opts : &g_gl_opts);
    strict_opts.v[50] = 1;
    const gl_opts* prev_opts = tl_gl_opts;
    tl_gl_opts = &strict_opts;                       // Run::gemm decides the third pass from the strict keys
    struct Restore { const gl_opts* p; ~Restore() { tl_gl_opts = p; } } restore{prev_opts};
    const size_t rows = (size_t)Bn * mo;             // rows of ONE chain; the token rows of the fuser are Bn * ng
    const int D = cfg.pos_out_dim;
    float* pin32 = e->f32("pn.in32", nch * rows * pin_dim);
    half_t* pins = e->h16("pn.ins", nch * rows * 2 * pin_dim);
    half_t* h1s = e->h16("pn.h1s", nch * rows * 2 * 512);
    half_t* h2s = e->h16("pn.h2s", nch * rows * 2 * 512);
    half_t* objss = e->h16("pn.objss", nch * rows * 2 * D);
    half_t* ctxs = e->h16("cond.ctxs", (size_t)Bn * Lc * 2 * ctx);
    CKP(pin32); CKP(pins); CKP(h1s); CKP(h2s); CKP(objss); CKP(ctxs);
    CK(posnet_input(e, in, Bn, true, pin32, st));
    CK(r.split(pin32, (int64_t)(nch * rows), pin_dim, pins));
    auto lin = [&](const half_t* a, int k, const std::string& w, void* out, int ldc, int out_mode, int epi, size_t m) {
        return r.gemm({a, 2 * k, true}, w, (int)m, out, ldc, {.out_mode = out_mode, .epi = epi});
    };
    for (int c = 0; c < nch; ++c) {                  // chain c on rows [c * rows, (c + 1) * rows) of every buffer
        const std::string pw = posnet_chain(cfg, c);
        const size_t o = c * rows;
        CK(lin(pins + o * 2 * pin_dim, pin_dim, pw + ".0", h1s + o * 2 * 512, 2 * 512, GL_OUT_F16_HILO, GL_EPI_SILU, rows));
        CK(lin(h1s + o * 2 * 512, 512, pw + ".2", h2s + o * 2 * 512, 2 * 512, GL_OUT_F16_HILO, GL_EPI_SILU, rows));
        CK(lin(h2s + o * 2 * 512, 512, pw + ".4", objss + o * 2 * D, 2 * D, GL_OUT_F16_HILO, GL_EPI_BIAS, rows));
    }
    if (ti) {                                        // objs = cat([objs_text, objs_image], dim=1): sample-major token rows
        half_t* cat = e->h16("pn.objss.cat", (size_t)Bn * ng * 2 * D);
        CKP(cat);
        cat_chains_kernel<<<dim3(256), dim3(256), 0, st>>>(reinterpret_cast<const uint32_t*>(objss), reinterpret_cast<uint32_t*>(cat), Bn, mo, D);
        GL_CHECK_LAUNCH();
        objss = cat;
    }
    const size_t tok = (size_t)Bn * ng;
    CK(r.split(context, (int64_t)Bn * Lc, ctx, ctxs));
    for (size_t li = 0; li < e->st_layers.size(); ++li) {
        const LayerD& l = e->st_layers[li];
        const std::string t = l.prefix + ".transformer_blocks.0";
        const std::string sl = std::to_string(li);
        const int C = l.cin, d = l.d_head;
        float* o32 = e->f32("hoist.objs32s." + sl, tok * C);
        CKP(o32);
        CK(lin(objss, D, t + ".fuser.linear", o32, C, GL_OUT_F32_ROWMAJOR, GL_EPI_BIAS, tok));
        half_t* kv = e->h16("hoist.kvctxs." + sl, (size_t)Bn * Lc * 4 * C);
        const int ldc_ = vt_ld(Lc);
        half_t* vt = e->h16("hoist.vtctxs." + sl, (size_t)2 * Bn * H * d * ldc_);
        CKP(kv); CKP(vt);
        CK(r.gemm({ctxs, 2 * ctx, true}, t + ".attn2.kv", Bn * Lc, kv, 4 * C, {.bias = false, .out_mode = GL_OUT_F16_HILO}));
        CK(r.transpose_v(kv + C, (int64_t)Lc * 4 * C, 4 * C, vt, ldc_, Bn, H, d, Lc));
        CK(r.transpose_v(kv + 3 * C, (int64_t)Lc * 4 * C, 4 * C, vt + (size_t)Bn * H * d * ldc_, ldc_, Bn, H, d, Lc));
    }
    e->strict_hoists_ok = true;
    e->strict_hoists_w3 = g_strict_w3;
    return 0;
}

namespace {
int set_conditioning(gl_engine* e, const float* context, const float* relations, const GroundIn& in, int32_t Bn, int32_t Lc, int32_t R, int32_t h,
                     int32_t w, void* stream) {
    if (!e || !e->wt.wbase || !context || Bn <= 0 || Lc <= 0 || h <= 0 || w <= 0) return GL_ERR_BAD_ARG;
    for (const KeptIn& k : kept_inputs(e->cfg, Bn)) if (in.*(k.field) == nullptr) return GL_ERR_BAD_ARG;      // every tensor the family reads
    const bool rel = e->cfg.no_relation == 0;
    if (rel && (!relations || R <= 0)) return GL_ERR_BAD_ARG;
    if (!rel) { relations = nullptr; R = 0; }       // a no_relation handle ignores both (R = 0 in its graph keys)
    gl_opts_scope opts_scope(e->ovr);       // this handle's option overrides are in effect for the call
    const gl_unet_config& cfg = e->cfg;
    hipStream_t st = (hipStream_t)stream;
    const int mo = cfg.max_objs, ng = n_ground(cfg), ctx = cfg.context_dim, H = cfg.num_heads;
    const bool ti = cfg.grounding == 1;
    const int nch = posnet_chains(cfg);
    if (Bn != e->Bn || Lc != e->Lc || R != e->R || h != e->lat_h || w != e->lat_w) e->cache.drop();     // shapes are part of the graph keys anyway
    if (h != e->lat_h || w != e->lat_w) e->extra_set = false;       // the inpainting extra was sized for the previous latent shape
    e->pool.changed = false;
    e->Bn = Bn; e->Lc = Lc; e->R = R; e->lat_h = h; e->lat_w = w;
    Run r{e, st, e->buf("splitk.ws", GL_WS_BYTES)};
    CKP(r.ws);
    // --- grounding tokens: PositionNet (text_grounding_net.py:26-43; keypoint_grounding_net.py:34-58: one chain over Bn * 17 P rows)
    const int pin_dim = pin_width(cfg);
    // (text_image_grounding_net.py:41-62: two chains, text then image, chain-major [nch, Bn * mo] rows until the final concatenation)
    const size_t crow = (size_t)Bn * mo;
    const int D = cfg.pos_out_dim;
    half_t* pin = e->h16("pn.in", nch * crow * pin_dim);
    half_t* h1 = e->h16("pn.h1", nch * crow * 512);
    half_t* h2 = e->h16("pn.h2", nch * crow * 512);
    half_t* objs = e->h16("pn.objs", nch * crow * D);
    half_t* ctx16 = e->h16("cond.ctx", (size_t)Bn * Lc * ctx);
    half_t* rel16 = rel ? e->h16("cond.rel", (size_t)Bn * R * ctx) : nullptr;
    CKP(pin); CKP(h1); CKP(h2); CKP(objs); CKP(ctx16);
    if (rel) CKP(rel16);
    if (cfg.grounding == 4) {       // spatial: the tokens are the tokenizer stage's output, fp32 -> the fp16 operand of fuser.linear
        f32_to_f16_kernel<<<dim3(64), dim3(256), 0, st>>>(in.tokens, objs, crow * D);
        GL_CHECK_LAUNCH();
    } else {
        CK(posnet_input(e, in, Bn, false, pin, st));
    }
    for (int c = 0; c < (cfg.grounding == 4 ? 0 : nch); ++c) {
        const std::string pw = posnet_chain(cfg, c);
        const size_t o = c * crow;
        CK(r.gemm({pin + o * pin_dim, pin_dim}, pw + ".0", Bn * mo, h1 + o * 512, 512, {.epi = GL_EPI_SILU}));
        CK(r.gemm({h1 + o * 512, 512}, pw + ".2", Bn * mo, h2 + o * 512, 512, {.epi = GL_EPI_SILU}));
        CK(r.gemm({h2 + o * 512, 512}, pw + ".4", Bn * mo, objs + o * D, D));
    }
    if (ti) {               // objs = cat([objs_text, objs_image], dim=1): sample b's ng token rows are [text (mo) | image (mo)]
        half_t* cat = e->h16("pn.objs.cat", (size_t)Bn * ng * D);
        CKP(cat);
        cat_chains_kernel<<<dim3(256), dim3(256), 0, st>>>(reinterpret_cast<const uint32_t*>(objs), reinterpret_cast<uint32_t*>(cat), Bn, mo, D / 2);
        GL_CHECK_LAUNCH();
        objs = cat;
    }
    f32_to_f16_kernel<<<dim3(256), dim3(256), 0, st>>>(context, ctx16, (size_t)Bn * Lc * ctx);
    if (rel) f32_to_f16_kernel<<<dim3(64), dim3(256), 0, st>>>(relations, rel16, (size_t)Bn * R * ctx);
    GL_CHECK_LAUNCH();
    for (size_t li = 0; li < e->st_layers.size(); ++li) {
        const LayerD& l = e->st_layers[li];
        const std::string t = l.prefix + ".transformer_blocks.0";
        const std::string sl = std::to_string(li);
        const int C = l.cin, d = l.d_head;
        // fuser.linear(objs) (attention.py:228)
        // (both forms are kept hoisted: fp32 rows for the precise mode's LayerNorm over [x ; objs], fp16 rows for the fp16-copy mode)
        half_t* o = e->h16("hoist.objs." + sl, (size_t)Bn * ng * C);
        float* o32 = e->f32("hoist.objs32." + sl, (size_t)Bn * ng * C);
        CKP(o); CKP(o32);
        CK(r.gemm({objs, D}, t + ".fuser.linear", Bn * ng, o, C));
        CK(r.gemm({objs, D}, t + ".fuser.linear", Bn * ng, o32, C, {.out_mode = GL_OUT_F32_ROWMAJOR}));
        // attn2 K/V of the text context (attention.py:124-125)
        half_t* kv = e->h16("hoist.kvctx." + sl, (size_t)Bn * Lc * 2 * C);
        const int ldc_ = vt_ld(Lc);
        half_t* vt = e->h16("hoist.vtctx." + sl, (size_t)Bn * H * d * ldc_);
        CKP(kv); CKP(vt);
        CK(r.gemm({ctx16, ctx}, t + ".attn2.kv", Bn * Lc, kv, 2 * C, {.bias = false}));
        CK(r.transpose_v(kv + C, (int64_t)Lc * 2 * C, 2 * C, vt, ldc_, Bn, H, d, Lc));
        if (!rel) continue;
        // rela_fuse K/V of the relation tokens (attention.py:348-349)
        half_t* kvr = e->h16("hoist.kvrel." + sl, (size_t)Bn * R * 2 * C);
        const int ldr_ = vt_ld(R);
        half_t* vtr = e->h16("hoist.vtrel." + sl, (size_t)Bn * H * d * ldr_);
        CKP(kvr); CKP(vtr);
        CK(r.gemm({rel16, ctx}, t + ".rela_fuse.attn.kv", Bn * R, kvr, 2 * C, {.bias = false}));
        CK(r.transpose_v(kvr + C, (int64_t)R * 2 * C, 2 * C, vtr, ldr_, Bn, H, d, R));
    }
    // --- strict mode's hoists: lazily (strict_hoists above).  A split_weights handle keeps the inputs they are computed from; they run now only
    //     when the handle is in strict mode at this point, else with the first strict forward
    e->strict_hoists_ok = false;
    if (cfg.split_weights) {
        float* cdst = e->f32("cond.in.context", (size_t)Bn * Lc * ctx);
        CKP(cdst);
        if (hipMemcpyAsync(cdst, context, (size_t)Bn * Lc * ctx * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
        for (const KeptIn& k : kept_inputs(cfg, Bn)) {
            float* dst = e->f32(k.tag, k.n);
            CKP(dst);
            if (hipMemcpyAsync(dst, in.*(k.field), k.n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
        }
        if (g_strict != 0) CK(strict_hoists(e, st));
    }
    // --- integer rectangles per transformer resolution (attention.py:321-346); none on a no_relation handle (they feed the relation chain alone)
    e->rel_slots = 0;
    if (rel) {
        std::vector<std::pair<int, int>> sides;
        int ch = h, cw = w;
        auto note = [&](int a, int b) { for (auto& v : sides) if (v.first == a && v.second == b) return; sides.push_back({a, b}); };
        for (auto& b : e->input_blocks)
            for (auto& l : b.layers) {
                if (l.kind == DOWN) { ch /= 2; cw /= 2; }
                else if (l.kind == ST) note(ch, cw);
            }
        note(ch, cw);
        for (auto& s : sides) {
            const std::string ss = level_tag(s.first, s.second);
            int* rects = reinterpret_cast<int*>(e->buf("cond.rects." + ss, (size_t)Bn * mo * 16));
            int* nvalid = reinterpret_cast<int*>(e->buf("cond.nvalid." + ss, (size_t)Bn * 4));
            int* poison = reinterpret_cast<int*>(e->buf("cond.poison." + ss, (size_t)Bn * 4));
            CKP(rects); CKP(nvalid); CKP(poison);
            rela_rects_kernel<<<dim3((Bn + 63) / 64), dim3(64), 0, st>>>(in.loc, in.masks, Bn, mo, s.first, s.second, rects, nvalid, poison);
            GL_CHECK_LAUNCH();
        }
        // Rows of the relation chain (attention.py:348-351 runs LN / cross-attention / FeedForward over all 30 rows of every sample; only
        // the first nvalid[b] of them enter the result, and the rows are independent of one another): the largest nvalid over samples and
        // resolutions, rounded up to 8.  One small device-to-host copy per conditioning (once per image batch, outside any capture).
        int slots = mo;
        if (g_rela_compact) {
            // every resolution's counts in flight, then ONE synchronisation
            std::vector<int> nv((size_t)Bn * sides.size());
            int mx = 0;
            for (size_t k = 0; k < sides.size(); ++k) {
                const int* nvalid = reinterpret_cast<const int*>(e->buf("cond.nvalid." + level_tag(sides[k].first, sides[k].second), (size_t)Bn * 4));
                CKP(nvalid);
                if (hipMemcpyAsync(nv.data() + k * Bn, nvalid, (size_t)Bn * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return GL_ERR_BAD_ARG;
            }
            if (hipStreamSynchronize(st) != hipSuccess) return GL_ERR_BAD_ARG;
            for (int v : nv) mx = v > mx ? v : mx;
            slots = (mx + 7) & ~7;
            if (slots < 8) slots = 8;
            if (slots > mo) slots = mo;
        }
        e->rel_slots = slots;          // part of the graph key: a rollout alternating between <= 8 and 9..16 boxes keeps both sets of graphs
    }
    if (e->pool.changed) e->cache.drop();
    e->cond_set = true;
    return 0;
}
}  // namespace

// the grounding family is a property of the handle: each family has its own conditioning entries
static int wrong_family(gl_engine* e, const char* entry, int want) {
    if (e->cfg.grounding == want) return 0;
    static const char* const made[5] = {"0 (text)", "1 (text_image)", "2 (keypoint)", "3", "4 (spatial)"};
    static const char* const use[5] = {"gl_set_conditioning / gl_set_conditioning_hw", "gl_set_conditioning_ti", "gl_set_conditioning_kp", "nothing",
                                       "gl_set_conditioning_tokens"};
    e->err = std::string(entry) + ": the handle was created with grounding = " + made[e->cfg.grounding] + "; use " + use[e->cfg.grounding];
    return GL_ERR_BAD_ARG;
}
// an axis that is not a multiple of 2^(number of downsamples) comes back shorter than the skip tensor it is concatenated with
static int check_hw(gl_engine* e, const char* entry, int h, int w) {
    int f = 1;
    for (auto& b : e->input_blocks) for (auto& l : b.layers) if (l.kind == DOWN) f *= 2;
    if (h <= 0 || w <= 0 || (h % f) != 0 || (w % f) != 0) {
        e->err = std::string(entry) + ": h = " + std::to_string(h) + ", w = " + std::to_string(w) + " must be positive multiples of " + std::to_string(f);
        return GL_ERR_BAD_ARG;
    }
    return 0;
}

extern "C" int gl_set_conditioning(gl_engine* e, const float* context, const float* relations, const float* boxes, const float* masks,
                                   const float* pos_emb, int32_t Bn, int32_t Lc, int32_t R, int32_t hw, void* stream) {
    if (!e) return GL_ERR_BAD_ARG;
    CK(wrong_family(e, "gl_set_conditioning", 0));
    return set_conditioning(e, context, relations, GroundIn{boxes, masks, pos_emb}, Bn, Lc, R, hw, hw, stream);
}

extern "C" int gl_set_conditioning_ti(gl_engine* e, const float* context, const float* relations, const float* boxes, const float* masks,
                                      const float* text_masks, const float* image_masks, const float* text_emb, const float* image_emb, int32_t Bn,
                                      int32_t Lc, int32_t R, int32_t h, int32_t w, void* stream) {
    if (!e) return GL_ERR_BAD_ARG;
    CK(wrong_family(e, "gl_set_conditioning_ti", 1));
    CK(check_hw(e, "gl_set_conditioning_ti", h, w));
    return set_conditioning(e, context, relations, GroundIn{boxes, masks, text_emb, text_masks, image_masks, image_emb}, Bn, Lc, R, h, w, stream);
}

extern "C" int gl_set_conditioning_hw(gl_engine* e, const float* context, const float* relations, const float* boxes, const float* masks,
                                      const float* pos_emb, int32_t Bn, int32_t Lc, int32_t R, int32_t h, int32_t w, void* stream) {
    if (!e) return GL_ERR_BAD_ARG;
    CK(wrong_family(e, "gl_set_conditioning_hw", 0));
    // every DOWN halves both axes and every UP doubles them back: an axis that is not a multiple of 2^(number of downsamples) comes back
    // shorter than the skip tensor it is concatenated with (the reference fails there too) -- rejected here, before anything is launched
    CK(check_hw(e, "gl_set_conditioning_hw", h, w));
    return set_conditioning(e, context, relations, GroundIn{boxes, masks, pos_emb}, Bn, Lc, R, h, w, stream);
}

extern "C" int gl_set_conditioning_kp(gl_engine* e, const float* context, const float* points, const float* masks, int32_t Bn, int32_t Lc, int32_t h,
                                      int32_t w, void* stream) {
    if (!e) return GL_ERR_BAD_ARG;
    CK(wrong_family(e, "gl_set_conditioning_kp", 2));
    CK(check_hw(e, "gl_set_conditioning_kp", h, w));
    return set_conditioning(e, context, nullptr, GroundIn{points, masks}, Bn, Lc, 0, h, w, stream);
}

extern "C" int gl_set_conditioning_tokens(gl_engine* e, const float* context, const float* objs, int32_t Bn, int32_t Lc, int32_t h, int32_t w,
                                          void* stream) {
    if (!e) return GL_ERR_BAD_ARG;
    CK(wrong_family(e, "gl_set_conditioning_tokens", 4));
    CK(check_hw(e, "gl_set_conditioning_tokens", h, w));
    GroundIn in;
    in.tokens = objs;
    return set_conditioning(e, context, nullptr, in, Bn, Lc, 0, h, w, stream);
}

// the extra channels of the GLIGEN first conv, by either family's entry: a pool buffer whose address the captured graphs read at replay time
static int set_extra(gl_engine* e, const std::string& entry, const float* extra, int32_t Bs, void* stream) {
    if (!e->cond_set) { e->err = entry + ": no conditioning call has fixed the latent shape yet"; return GL_ERR_BAD_ARG; }
    if (!extra || Bs < 1 || Bs > e->Bn) { e->err = entry + ": extra must be a device pointer to Bs = 1 or Bn / reps samples"; return GL_ERR_BAD_ARG; }
    const size_t n = (size_t)Bs * extra_channels(e->cfg, e->ground_extra) * e->lat_h * e->lat_w;
    e->pool.changed = false;
    float* dst = e->f32("in.extra", n);
    CKP(dst);
    // the captured graphs hold this buffer's address and the broadcast flag of the pack launch: a moved buffer or another Bs makes them stale
    if (e->pool.changed || (e->extra_set && Bs != e->extra_bs)) { e->cache.drop(); e->pool.changed = false; }
    if (hipMemcpyAsync(dst, extra, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return GL_ERR_BAD_ARG;
    e->extra_bs = Bs;
    e->extra_set = true;
    return 0;
}

extern "C" int gl_set_inpaint_extra(gl_engine* e, const float* extra, int32_t Bs, void* stream) {
    if (!e) return GL_ERR_BAD_ARG;
    if (!e->cfg.inpaint_mode) { e->err = "gl_set_inpaint_extra: the handle was created with inpaint_mode = 0 (its first conv reads the latent alone)"; return GL_ERR_BAD_ARG; }
    return set_extra(e, "gl_set_inpaint_extra", extra, Bs, stream);
}

extern "C" int gl_set_extra_channels(gl_engine* e, int32_t channels) {
    if (!e) return GL_ERR_BAD_ARG;
    if (e->cfg.grounding != 4) {
        e->err = "gl_set_extra_channels: only a spatial handle (grounding = 4) has a grounding downsampler in front of its first conv";
        return GL_ERR_UNSUPPORTED;
    }
    if (channels < 0 || e->cfg.in_channels + channels > CIN_PAD) {
        e->err = "gl_set_extra_channels: in_channels + channels must fit the first conv's " + std::to_string(CIN_PAD) + " padded input channels";
        return GL_ERR_UNSUPPORTED;
    }
    if (channels != e->ground_extra) {       // the pack launch of the captured graphs and the extra buffer's size follow the count
        e->cache.drop();
        e->extra_set = false;
    }
    e->ground_extra = channels;
    return 0;
}

extern "C" int gl_set_grounding_extra(gl_engine* e, const float* extra, int32_t Bs, void* stream) {
    if (!e) return GL_ERR_BAD_ARG;
    if (e->ground_extra == 0) {
        e->err = "gl_set_grounding_extra: the handle has no extra channels (gl_set_extra_channels): its first conv reads the latent alone";
        return GL_ERR_BAD_ARG;
    }
    return set_extra(e, "gl_set_grounding_extra", extra, Bs, stream);
}

extern "C" int gl_unet_forward(gl_engine* e, const float* x, const float* t_dev, float t_host, int32_t reps, float fuser_scale, int32_t sd_conv,
                               float* eps, int32_t use_graph, void* stream) {
    if (!e || !e->cond_set || !x || !eps || reps < 1 || (e->Bn % reps) != 0) return GL_ERR_BAD_ARG;
    if (e->cfg.inpaint_mode) {              // host-side checks, before anything is launched
        if (sd_conv) { e->err = "gl_unet_forward: sd_conv != 0 on an inpaint_mode handle (its first conv is not restorable)"; return GL_ERR_BAD_ARG; }
        if (!e->extra_set) { e->err = "gl_unet_forward: an inpaint_mode handle needs gl_set_inpaint_extra after the conditioning call that fixed (h, w)"; return GL_ERR_BAD_ARG; }
        if (e->extra_bs != 1 && e->extra_bs != e->Bn / reps) {
            e->err = "gl_unet_forward: the inpainting extra has " + std::to_string(e->extra_bs) + " samples, the latent " + std::to_string(e->Bn / reps);
            return GL_ERR_BAD_ARG;
        }
    }
    if (e->ground_extra != 0 && !sd_conv) {      // a spatial handle on its GLIGEN conv: the same host-side checks
        if (!e->extra_set) { e->err = "gl_unet_forward: sd_conv = 0 on a handle with extra channels needs gl_set_grounding_extra after the conditioning call that fixed (h, w)"; return GL_ERR_BAD_ARG; }
        if (e->extra_bs != 1 && e->extra_bs != e->Bn / reps) {
            e->err = "gl_unet_forward: the grounding extra has " + std::to_string(e->extra_bs) + " samples, the latent " + std::to_string(e->Bn / reps);
            return GL_ERR_BAD_ARG;
        }
    }
    gl_opts_scope opts_scope(e->ovr);       // this handle's option overrides are in effect for the call
    if (sd_conv && !e->has_sd) return GL_ERR_BAD_ARG;
    const gl_unet_config& cfg = e->cfg;
    hipStream_t st = (hipStream_t)stream;
    const int Bn = e->Bn;
    const size_t hw = (size_t)e->lat_h * e->lat_w;
    const size_t nx = (size_t)(Bn / reps) * cfg.in_channels * hw;
    const size_t ne = (size_t)Bn * cfg.out_channels * hw;
    e->pool.changed = false;
    float* x_lat = e->f32("in.xlat", nx);
    float* t_buf = e->f32("in.t", Bn);
    float* eps_i = e->f32("out.eps", ne);
    CKP(x_lat); CKP(t_buf); CKP(eps_i);
    if (x != x_lat && hipMemcpyAsync(x_lat, x, nx * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    if (t_dev) {
        if (hipMemcpyAsync(t_buf, t_dev, (size_t)Bn * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    } else {
        fill_f32_kernel<<<dim3((Bn + 255) / 256), dim3(256), 0, st>>>(t_buf, t_host, Bn);
        GL_CHECK_LAUNCH();
    }
    CK(set_fuser_scale(e, fuser_scale, st));
    if (g_strict != 0 && cfg.split_weights && (!e->strict_hoists_ok || e->strict_hoists_w3 != g_strict_w3)) {
        // first strict forward since the conditioning was set (or since key 51 changed): the split-fp16 hoists, on the caller's stream, before any
        // capture; their buffers are new to the pool the first time, which makes the captured graphs stale
        CK(strict_hoists(e, st));
        if (e->pool.changed) { e->cache.drop(); e->pool.changed = false; }
    }
    const bool fuser_on = fuser_scale != 0.0f || g_force_fuser != 0;
    e->cache.sync_epochs(e->ovr);
    const bool uniform_t = t_dev == nullptr;
    const GraphKey key{Bn, e->lat_h, e->lat_w, e->R, e->Lc, fuser_on, sd_conv != 0, reps, uniform_t, e->rel_slots, cfg.no_relation != 0};
    CK(e->cache.run(key, use_graph != 0, st, e->pool,
                    [&](hipStream_t s, int* nl) { return launch_forward(e, reps, fuser_on, sd_conv != 0, uniform_t, s, nl); }, &e->launches));
    if (eps != eps_i && hipMemcpyAsync(eps, eps_i, ne * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return GL_ERR_BAD_ARG;
    return 0;
}

// What every sampler step does first, behind the entry's own pointer checks: the handle's option overrides, the reps check, the refusal of a
// model whose output is no latent, then eps = UNet(x, t) into the handle's own ``out.eps``.  Hands back that buffer and n = its elements / reps,
// the size of the latent.  ``a``: any of the step structs (they share the fields read here).  ``min_reps`` .. ``max_reps``: the batch multiples
// the entry takes -- 1 and 2 for the three sampler steps, 3 alone for gl_cfg3_eval.  The option scope ends with the forward: the update
// launches behind it read no option.
template <typename Args>
static int step_eval(gl_engine* e, const Args* a, const float* x, void* stream, float** eps_i, size_t* n, int min_reps = 1, int max_reps = 2) {
    gl_opts_scope opts_scope(e->ovr);       // this handle's option overrides are in effect for the call
    if (a->reps < min_reps || a->reps > max_reps) return GL_ERR_BAD_ARG;
    const gl_unet_config& cfg = e->cfg;
    if (cfg.in_channels != cfg.out_channels) return GL_ERR_UNSUPPORTED;
    const size_t ne = (size_t)e->Bn * cfg.out_channels * e->lat_h * e->lat_w;
    *eps_i = e->f32("out.eps", ne);
    CKP(*eps_i);
    *n = ne / a->reps;
    return gl_unet_forward(e, x, nullptr, a->t, a->reps, a->fuser_scale, a->sd_conv, *eps_i, a->use_graph, stream);
}

extern "C" int gl_plms_step(gl_engine* e, const gl_plms_step_args* a, void* stream) {
    if (!e || !a || !a->x_eval || !a->x_base || !a->x_out || !a->e_out || a->n_terms < 1 || a->n_terms > 4) return GL_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* eps_i;
    size_t n;
    CK(step_eval(e, a, a->x_eval, stream, &eps_i, &n));
    if (a->reps == 2) {
        CK(gl_cfg_combine(eps_i, a->guidance, (int64_t)n, a->e_out, st));
    } else if (hipMemcpyAsync(a->e_out, eps_i, n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        return GL_ERR_BAD_ARG;
    }
    const float* t[4] = {nullptr, nullptr, nullptr, nullptr};
    float c[4] = {0, 0, 0, 0};
    for (int j = 0; j < a->n_terms; ++j) { t[j] = a->e_terms[j]; c[j] = a->coef[j]; }
    if (!t[0]) return GL_ERR_BAD_ARG;
    return gl_plms_update(a->x_base, t[0], t[1], t[2], t[3], c[0], c[1], c[2], c[3], a->div, a->sqrt_at, a->s1m, a->sqrt_aprev, a->dir_coef,
                          (int64_t)n, a->x_out, st);
}

extern "C" int gl_ddim_step(gl_engine* e, const gl_ddim_step_args* a, void* stream) {
    if (!e || !a || !a->x || !a->x_out) return GL_ERR_BAD_ARG;
    float* eps_i;
    size_t n;
    CK(step_eval(e, a, a->x, stream, &eps_i, &n));
    // the CFG combine, pred_x0 and x_prev in one launch, straight from the 2B output
    return gl_ddim_update(eps_i, a->x, a->noise, a->reps, a->guidance, a->sqrt_at, a->s1m, a->sqrt_aprev, a->dir_coef, a->sigma,
                          (int64_t)n, a->x_out, a->pred_x0, stream);
}

extern "C" int gl_dpmpp_step(gl_engine* e, const gl_dpmpp_step_args* a, void* stream) {
    if (!e || !a || !a->x || !a->x_out || !a->x0_out) return GL_ERR_BAD_ARG;
    if (!a->x0_old && a->w0 != 0.0f) return GL_ERR_BAD_ARG;       // refused before the forward runs and ahead of the channel refusal
    float* eps_i;
    size_t n;
    CK(step_eval(e, a, a->x, stream, &eps_i, &n));
    // the CFG combine, the x0 prediction, the multistep difference and x_prev in one launch, straight from the 2B output
    return gl_dpmpp_update(eps_i, a->x, a->x0_old, a->reps, a->guidance, a->sqrt_at, a->s1m, a->c_x, a->c_d, a->w1, a->w0,
                           (int64_t)n, a->x_out, a->x0_out, stream);
}

extern "C" int gl_cfg3_eval(gl_engine* e, const gl_cfg3_eval_args* a, void* stream) {
    if (!e || !a || !a->x || !a->e_out) return GL_ERR_BAD_ARG;
    if (e->cond_set && (e->Bn % 3) != 0) {
        e->err = "gl_cfg3_eval: the conditioning batch has " + std::to_string(e->Bn) + " samples, no multiple of 3 ([cond ; text-only ; uncond])";
        return GL_ERR_BAD_ARG;
    }
    float* eps_i;
    size_t n;
    CK(step_eval(e, a, a->x, stream, &eps_i, &n, 3, 3));
    // the thirds of the handle's own output -> the guided eps the caller's update reads
    return gl_cfg3_combine(eps_i, a->s_text, a->s_layout, (int64_t)n, a->e_out, stream);
}

extern "C" int gl_set_handle_option(gl_engine* e, int key, int value) {
    return e ? gl_handle_set_option(e->ovr, key, value) : GL_ERR_BAD_ARG;
}

extern "C" int gl_clear_handle_options(gl_engine* e) {
    if (!e) return GL_ERR_BAD_ARG;
    e->ovr.mask = 0;
    ++e->ovr.epoch;
    return 0;
}

extern "C" int gl_last_error(const gl_engine* e, char* dst, int32_t bytes) {
    if (!dst || bytes <= 0) return GL_ERR_BAD_ARG;
    const std::string hl = e ? std::string() : std::string(gl_handleless_error());   // no handle: the entries that take none
    const std::string& err = e ? e->err : hl;
    const size_t n = err.size() < (size_t)bytes - 1 ? err.size() : (size_t)bytes - 1;
    memcpy(dst, err.data(), n);
    dst[n] = 0;
    return (int)err.size();
}

extern "C" int64_t gl_pool_bytes(const gl_engine* e) {
    return e ? e->pool.bytes() : -1;
}
extern "C" int gl_num_launches(const gl_engine* e) { return e ? e->launches : GL_ERR_BAD_ARG; }
extern "C" int gl_sizeof_unet_config(void) { return (int)sizeof(gl_unet_config); }
extern "C" int gl_sizeof_weight_info(void) { return (int)sizeof(gl_weight_info); }
extern "C" int gl_sizeof_plms_step_args(void) { return (int)sizeof(gl_plms_step_args); }
extern "C" int gl_sizeof_ddim_step_args(void) { return (int)sizeof(gl_ddim_step_args); }
extern "C" int gl_sizeof_dpmpp_step_args(void) { return (int)sizeof(gl_dpmpp_step_args); }
extern "C" int gl_sizeof_cfg3_eval_args(void) { return (int)sizeof(gl_cfg3_eval_args); }
