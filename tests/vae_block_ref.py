"""CPU references for the VAE stage's blocks and the shapes at which its kernels are tested (no GPU import).

``resnet_block`` / ``attn_block`` restate ``_VAEStage._resnet`` / ``_attn`` (layoutllm_t2i_amd/vae.py) from the PACKED weights of a stage
(``dec.W``: 3x3 convs fp16 [Cout, 9 Cin] in pack_conv3x3's K order, 1x1 convs fp16 [N, K], C^-0.5 folded into q, norm affine and biases
fp32), so a comparison against them sees kernel error only, never packing error.  ``round_points=True`` rounds the activations to fp16 exactly
where the engine stores fp16 (after each GroupNorm(+SiLU), after conv1, after the shortcut, at the block output; in the attention block also
q, k, v, the logits, P and o); ``round_points=False`` is the plain block.  ``dtype`` is the arithmetic: float64 for the reference, float32 for
the "reference alone" checks of tests/test_vae_block_ref_host.py (what CPU fp32 arithmetic alone does to a comparison).

The case lists below are shared by tests/test_vae_block_ref_host.py (CPU) and tests/test_gpu_vae_kernels.py (GPU).
"""
from __future__ import annotations

import math
from typing import Dict, Mapping, Tuple

import torch
import torch.nn.functional as F

from layoutllm_t2i_amd import recipe
from layoutllm_t2i_amd.arch import VAE_TINY, VAEConfig, vae_decoder_param_shapes, vae_encoder_param_shapes

F64 = torch.float64
EPS = 1e-6                      # GroupNorm eps of the VAE (model.py:38-39)
B = 3                           # batch of every case but the attention chain's: a wrong batch stride shows in rows 1 and 2
MAP = (12, 20)                  # rectangular map of the GEMM / conv / block cases: 240 pixels, M = 720 rows at B = 3

# ------------------------------------------------------------------------------------------------------------------ cases
# GroupNorm (C, HW).  C = 64 / 128 / 256 / 512 are 2 / 4 / 8 / 16 channels per group; with C = 64 / 128 an 8-channel vector spans 4 / 2
# groups.  HW = 130: 32 chunks of 5 pixels, 26 used, 6 empty.  4096: the last size with 64 chunks.  4100: 8 chunks of 513, the last 509.
# 33856 (184 x 184): 66 chunks of 513, the last 511.  768|769, 1280|1281, 2560|2561 (C = 256) and 384|385, 1280|1281 (C = 512): the
# register-resident kernel's 3 -> 5 -> 10 vectors-per-thread switch points and its hand-over to statistics + apply.
GN_CASES = [(64, 130),
            (128, 130), (128, 4096), (128, 4100), (128, 33856),
            (256, 768), (256, 769), (256, 1280), (256, 1281), (256, 2560), (256, 2561), (256, 4100),
            (512, 384), (512, 385), (512, 1280), (512, 1281), (512, 4100)]
GN_SHARP_CASES = [(128, 4100), (128, 33856), (128, 130), (256, 2561), (512, 1281)]
GN_SHARP_TOL = (2e-5, 2e-6)     # tests/test_gpu_kernels.py::test_groupnorm_fp32_stream_hilo_and_raw_split


def gn_single_launch(C: int, HW: int) -> bool:
    """what csrc/norms.hip documents for these widths: whole 8-channel vectors per group (C % 256 == 0) and at most 2560 vectors per
    (sample, group) take the register-resident single-launch kernel; C = 64 / 128 (fewer than 8 channels per group) never do"""
    return C % 256 == 0 and HW * (C // 256) <= 2560


def gn_chunks(HW: int, nchunk: int) -> Tuple[int, int, int]:
    """(pixels per chunk, pixels of the last non-empty chunk, empty chunks) of a map cut into ``nchunk`` ceil-sized chunks"""
    ppc = -(-HW // nchunk)
    used = -(-HW // ppc)
    return ppc, HW - (used - 1) * ppc, nchunk - used


# mid-attention chain (C, N): N = 144 -> Np = 192 (zero-padded keys); N = 2112 = 2048 + 64: softmax_rows' 2048-wide loop runs twice
ATTN_CASES = [(512, 64), (512, 144), (512, 2112), (128, 144)]
ATTN_B = 2
ATTN_HARD_CASE = (512, 144)
ATTN_HARD_ROWMAX = 40.0
ATTN_TOL = (2e-3, 2e-4)         # the project's attention tolerance (tests/test_gpu_kernels.py)
# Whole chain against EXACT fp64 attention.  The rounded model (fp16 logits, P and o) evaluated in CPU fp32 sits at 2.28 / 2.02 / 0.58 / 0.54
# of ATTN_TOL at logit standard deviations 2 / 1 / 0.5 / 0.25 (worst of ATTN_CASES; the same in fp64 arithmetic: it is the model's three
# roundings, the final one alone is 0.245): no scale gives the 4x margin, below 0.5 the figure stops falling.  So: the scale is 0.5, the
# CPU-fp32 figure 0.58, and the comparison's tolerance 4 x 0.58 of ATTN_TOL.
ATTN_CHAIN_LOGIT_STD = 0.5
ATTN_CHAIN_CPU_FIGURE = 0.58

GEMM_BIAS_CASES = [(128, 256), (256, 512), (512, 512), (256, 128), (512, 256)]      # (N, K), M = 720
GEMM_RES_CASE = (512, 512)
CONV_CASES = [(512, 512), (512, 256), (256, 256), (256, 128), (128, 128), (128, 256), (256, 512)]      # (Cin, Cout), bias
CONV_RES_CASES = [(256, 128), (128, 128)]
CONV_OUT_CASES = [(128, 3), (512, 8)]
CONV_OUT_TOL = (1e-4, 1e-5)     # tests/test_gpu_kernels.py::test_conv3x3_first_and_last (conv_last_nchw_f32)
CONV_MANY_TILES = (128, 128, 100, 108)          # Cin, Cout, h, w at B = 1: 10800 rows = 42 tiles of 256 rows + 48

# (stage, config, block prefix, cin, cout)
RESNET_CASES = [("dec", "full", "decoder.mid.block_1", 512, 512), ("dec", "full", "decoder.up.1.block.0", 512, 256),
                ("dec", "full", "decoder.up.1.block.1", 256, 256), ("dec", "full", "decoder.up.0.block.0", 256, 128),
                ("dec", "full", "decoder.up.0.block.1", 128, 128),
                ("enc", "full", "encoder.down.1.block.0", 128, 256), ("enc", "full", "encoder.down.2.block.0", 256, 512)]
ATTN_BLOCK_CASES = [("dec", "full", "decoder.mid.attn_1", 512), ("dec", "tiny", "decoder.mid.attn_1", 128)]
KERNEL_TOL = (1e-3, 1e-4)      # tests/test_gpu_kernels.py: rtol 1e-3, atol 1e-4 x max(1, max|ref|), zero violators
BLOCK_TOL = KERNEL_TOL
# Blocks against the rounded fp64 model.  The rounded model in CPU fp32 does NOT pass BLOCK_TOL with a 4x margin at any input scale: an fp16
# rounding that falls the other way is a whole fp16 ulp (up to 9.8e-4 relative) at the block output, and where a block has a 1x1 shortcut
# such a flip of the shortcut (an ulp of a value of 2..8) lands on outputs where shortcut and conv2 cancel.  CPU-fp32 figures, as fractions
# of BLOCK_TOL, the largest over the library's summation order and six permuted K orders of every conv / 1x1 conv (they do not move with
# the thread count): resnet blocks with cin == cout 0.86, with a shortcut 1.56 (0.72 .. 1.56 over the orders), attention blocks 0.94.
# Each comparison's tolerance is 4 x its figure x BLOCK_TOL (block_tol()).
BLOCK_CPU_FIGURE = {"resnet": 0.86, "resnet_shortcut": 1.56, "attn": 0.94}
CONFIGS = {"full": VAEConfig(), "tiny": VAE_TINY}


def widened(tol: Tuple[float, float], cpu_figure: float) -> Tuple[float, float]:
    """the issue's rule: a comparison the CPU-fp32 evaluation of its own reference model passes with a 4x margin (figure <= 0.25) keeps
    ``tol``; otherwise its tolerance is 4 x the CPU-fp32 figure"""
    f = 1.0 if cpu_figure <= 0.25 else 4.0 * cpu_figure
    return tol[0] * f, tol[1] * f


def block_kind(cin=None, cout=None) -> str:
    return "attn" if cin is None else "resnet" if cin == cout else "resnet_shortcut"


def block_tol(kind: str) -> Tuple[float, float]:
    return widened(BLOCK_TOL, BLOCK_CPU_FIGURE[kind])


def attn_chain_tol() -> Tuple[float, float]:
    return widened(ATTN_TOL, ATTN_CHAIN_CPU_FIGURE)


# ------------------------------------------------------------------------------------------------------------------ inputs
def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(recipe.normal(f"vaek.{tag}", tuple(shape), 17)) * scale


def r16(x, on=True):
    """x rounded to fp16, in x's dtype"""
    return x.to(torch.float16).to(x.dtype) if on else x


def gn_input(C: int, HW: int, large_mean: bool = False) -> torch.Tensor:
    """fp32 [B * HW, C].  The pixel ramp gives every chunk of a map another mean, so a chunk merged with a wrong weight moves the
    result.  ``large_mean``: per-channel means of +30 / -30 (alternating, so every group holds both) at std 0.5."""
    x = rnd(f"gn{C}.{HW}.{int(large_mean)}", (B * HW, C))
    ramp = torch.linspace(-1.0, 1.0, HW).repeat(B)[:, None]
    if large_mean:
        sign = torch.where(torch.arange(C) % 2 == 0, 30.0, -30.0)[None, :]
        return x * 0.5 + sign + 0.25 * ramp
    return x * 1.5 + 0.3 + 0.5 * ramp


def gn_affine(C: int):
    return 1 + 0.1 * rnd(f"gng{C}", (C,)), 0.1 * rnd(f"gnb{C}", (C,))


def attn_inputs(C: int, N: int, logit_std: float):
    """fp16-rounded q, k, v [ATTN_B * N, C] (fp32 tensors) with logits q.k of the given standard deviation"""
    q = r16(rnd(f"aq{C}.{N}", (ATTN_B * N, C)) * (logit_std / math.sqrt(C)))
    k = r16(rnd(f"ak{C}.{N}", (ATTN_B * N, C)))
    v = r16(rnd(f"av{C}.{N}", (ATTN_B * N, C)))
    return q, k, v


def attn_hard_inputs(C: int, N: int):
    """the same with q scaled so that the median row maximum of the exact logits is ATTN_HARD_ROWMAX"""
    q, k, v = attn_inputs(C, N, 1.0)
    rowmax = torch.stack([(q[b * N:(b + 1) * N].double() @ k[b * N:(b + 1) * N].double().T).max(dim=1).values for b in range(ATTN_B)])
    return r16(q * float(ATTN_HARD_ROWMAX / rowmax.median())), k, v


def gemm_operands(N: int, K: int, M: int):
    """fp16-rounded a [M, K] and w [N, K], fp32 bias [N]"""
    return r16(rnd(f"ga{M}.{K}", (M, K))), r16(rnd(f"gw{N}.{K}", (N, K), 1 / math.sqrt(K))), rnd(f"gb{N}.{K}", (N,), 0.1)


def conv_operands(cin: int, cout: int, Bn: int, sh: int, sw: int):
    """fp16-rounded NHWC rows x [Bn * sh * sw, cin] and w [cout, cin, 3, 3], fp32 bias [cout]"""
    return (r16(rnd(f"cx{cin}.{Bn}.{sh}", (Bn * sh * sw, cin))), r16(rnd(f"cw{cin}.{cout}", (cout, cin, 3, 3), 1 / math.sqrt(9 * cin))),
            rnd(f"cb{cin}.{cout}", (cout,), 0.1))


def block_input(tag: str, rows: int, C: int) -> torch.Tensor:
    return r16(rnd(f"bx.{tag}", (rows, C)) * 1.2 + 0.2)


# ------------------------------------------------------------------------------------------------------------------ weights
def block_state(cfgname: str, prefix: str, encoder: bool) -> Tuple[Dict[str, object], Dict[str, Tuple[int, ...]]]:
    """recipe tensors (reference names, fp32) and shapes of one block of a stage: what VAEDecoder / VAEEncoder get for it"""
    cfg = CONFIGS[cfgname]
    shapes = (vae_encoder_param_shapes if encoder else vae_decoder_param_shapes)(cfg)
    need = {n: s for n, s in shapes.items() if n.startswith(prefix + ".")}
    assert need, prefix
    return {n: recipe.tensor("vae." + n, s, 0) for n, s in need.items()}, need


def pack_exact(sd: Mapping[str, object], need: Mapping[str, Tuple[int, ...]]) -> Dict[str, torch.Tensor]:
    """vae._pack's layouts WITHOUT its fp16 rounding, in fp64 (q fold included): the weights of the plain fp64 block"""
    W: Dict[str, torch.Tensor] = {}
    for name, shp in need.items():
        if not name.endswith(".weight"):
            continue
        p = name[:-7]
        w, b = torch.as_tensor(sd[name]).double(), torch.as_tensor(sd[p + ".bias"]).double()
        if len(shp) == 1:
            W[p + ".g"], W[p + ".b"] = w, b
            continue
        if shp[2] == 3:
            cout, cin = shp[0], shp[1]
            W[p + ".w"] = w.reshape(cout, cin // 64, 64, 3, 3).permute(0, 1, 3, 4, 2).reshape(cout, -1)
        else:
            s = float(shp[0]) ** -0.5 if p.endswith("attn_1.q") else 1.0
            W[p + ".w"], b = w.reshape(shp[0], shp[1]) * s, b * s
        W[p + ".b"] = b
    return W


def unpack_conv3x3(wp: torch.Tensor, dtype) -> torch.Tensor:
    """packed [Cout, 9 Cin] (K = 64-channel block, tap, channel in block) -> [Cout, Cin, 3, 3]"""
    cout, k = wp.shape
    cin = k // 9
    return wp.detach().cpu().to(dtype).reshape(cout, cin // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(cout, cin, 3, 3).contiguous()


def _w(W, name, dtype):
    return W[name].detach().cpu().to(dtype)


# ------------------------------------------------------------------------------------------------------------------ ops
def group_norm(x, gamma, beta, Bn: int, HW: int, silu: bool, eps: float = EPS):
    """GroupNorm(32) (+ SiLU) of NHWC rows x [Bn * HW, C], in x's dtype"""
    C = x.shape[1]
    y = F.group_norm(x.view(Bn, HW, C).permute(0, 2, 1), 32, gamma.to(x.dtype), beta.to(x.dtype), eps)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1).reshape(Bn * HW, C)


def conv3x3(x, w4, bias, Bn: int, sh: int, sw: int):
    """3x3 / pad 1 conv of NHWC rows x [Bn * sh * sw, Cin] -> rows [Bn * sh * sw, Cout]"""
    y = F.conv2d(x.view(Bn, sh, sw, -1).permute(0, 3, 1, 2), w4, bias, padding=1)
    return y.permute(0, 2, 3, 1).reshape(Bn * sh * sw, -1)


def nchw(rows, Bn: int, sh: int, sw: int):
    return rows.view(Bn, sh, sw, -1).permute(0, 3, 1, 2).contiguous()


def nhwc_rows(x):
    Bn, C, sh, sw = x.shape
    return x.permute(0, 2, 3, 1).reshape(Bn * sh * sw, C).contiguous()


def attention(q, k, v, Bn: int, N: int, round_points: bool):
    """softmax(q k^T) v per sample on rows [Bn * N, C] (the scale is already in q); ``round_points``: logits, P and o through fp16"""
    outs = []
    for b in range(Bn):
        s = slice(b * N, (b + 1) * N)
        logits = r16(q[s] @ k[s].T, round_points)
        p = r16(torch.softmax(logits, dim=-1), round_points)
        outs.append(r16(p @ v[s], round_points))
    return torch.cat(outs, 0)


# ------------------------------------------------------------------------------------------------------------------ blocks
def resnet_block(W, p: str, x, Bn: int, sh: int, sw: int, round_points: bool, dtype=F64):
    """_VAEStage._resnet on rows x [Bn * sh * sw, cin]"""
    rp, HW = round_points, sh * sw
    x = x.detach().cpu().to(dtype)
    t = r16(group_norm(x, _w(W, p + ".norm1.g", dtype), _w(W, p + ".norm1.b", dtype), Bn, HW, True), rp)
    h = r16(conv3x3(t, unpack_conv3x3(W[p + ".conv1.w"], dtype), _w(W, p + ".conv1.b", dtype), Bn, sh, sw), rp)
    t2 = r16(group_norm(h, _w(W, p + ".norm2.g", dtype), _w(W, p + ".norm2.b", dtype), Bn, HW, True), rp)
    sk = x
    if (p + ".nin_shortcut.w") in W:
        sk = r16(F.linear(x, _w(W, p + ".nin_shortcut.w", dtype), _w(W, p + ".nin_shortcut.b", dtype)), rp)
    return r16(conv3x3(t2, unpack_conv3x3(W[p + ".conv2.w"], dtype), _w(W, p + ".conv2.b", dtype), Bn, sh, sw) + sk, rp)


def attn_block(W, p: str, x, Bn: int, N: int, round_points: bool, dtype=F64):
    """_VAEStage._attn on rows x [Bn * N, C]"""
    rp = round_points
    x = x.detach().cpu().to(dtype)
    hn = r16(group_norm(x, _w(W, p + ".norm.g", dtype), _w(W, p + ".norm.b", dtype), Bn, N, False), rp)
    q, k, v = (r16(F.linear(hn, _w(W, f"{p}.{n}.w", dtype), _w(W, f"{p}.{n}.b", dtype)), rp) for n in "qkv")
    o = attention(q, k, v, Bn, N, rp)
    return r16(F.linear(o, _w(W, p + ".proj_out.w", dtype), _w(W, p + ".proj_out.b", dtype)) + x, rp)


# ------------------------------------------------------------------------------------------------------------------ comparison
def worst_ratio(out, ref, rtol: float, atol: float) -> float:
    """max over the elements of |out - ref| / (atol * max(1, max|ref|) + rtol * |ref|): the tolerance test of test_gpu_kernels.check
    passes with zero violators iff this is <= 1, and with an n-fold margin iff it is <= 1 / n"""
    out, ref = out.double(), ref.double()
    scale = max(1.0, float(ref.abs().max()))
    return float(((out - ref).abs() / (atol * scale + rtol * ref.abs())).max())
