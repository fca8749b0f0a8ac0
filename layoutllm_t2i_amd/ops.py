"""Host-side wrappers: torch tensors (device memory + streams only) -> raw pointers -> C ABI.

Each function launches exactly one HIP kernel from libgligen_hip.so on torch's current stream.
There is no eager/PyTorch fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_GATE_RES, EPI_GEGLU, EPI_RES, EPI_ROWBIAS, EPI_SILU, OUT_F16_HILO, OUT_F16_ROWMAJOR, OUT_F32_NCHW,
                   OUT_F32_ROWMAJOR, AttnArgs, ConvArgs, GemmArgs, GnArgs, check)

F16 = torch.float16
F32 = torch.float32


_DEV = None


def _stream() -> int:
    """Stream of the device the last checked tensor lives on (``_req`` records it and asserts that all tensors of a
    call share it).  A tensor on cuda:N while another device is current therefore launches on cuda:N's current stream."""
    dev = _DEV if _DEV is not None else torch.cuda.current_device()
    if dev != torch.cuda.current_device():
        raise _lib.HipLibraryError(f"tensors live on cuda:{dev} but cuda:{torch.cuda.current_device()} is current: wrap the "
                                   "call in torch.cuda.device(...) (kernels launch on the current device)")
    _lib.init_device(dev)
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str, align: int = 16) -> None:
    if not t.is_cuda:
        raise _lib.HipLibraryError(f"{name}: tensor is not on the GPU (the HIP path has no CPU fallback)")
    global _DEV
    _DEV = t.device.index
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.data_ptr() % align:
        raise ValueError(f"{name}: pointer not {align}-byte aligned")


def _rows(t: torch.Tensor, name: str):
    """2-D row view: returns (rows, cols, row_stride) requiring unit column stride."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D tensor with contiguous columns, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


_WS = {}
WORKSPACE_BYTES = 96 << 20


def _workspace(device) -> torch.Tensor:
    """Per-device split-K scratch (fp32 partial tiles); allocated once so captured graphs stay valid."""
    key = (device.type, device.index)
    t = _WS.get(key)
    if t is None:
        t = torch.empty(WORKSPACE_BYTES // 4, dtype=F32, device=device)
        _WS[key] = t
    return t


def _fill_epilogue(g: GemmArgs, epi, out, N_out, bias, res, gate, rowbias, rows_per_sample, nchw_hw, out16=None, hilo_out=False):
    """``out`` fp16 [M, N] (plain), fp32 [M, N] (residual stream; ``out16`` = optional fp16 copy) or, with ``nchw_hw``,
    fp32 NCHW; ``hilo_out``: fp16 [M, 2N] = [hi | lo] (GL_OUT_F16_HILO).  ``res`` may be fp16 or fp32 (residual stream)."""
    ws = _workspace(out.device)
    g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    g.bias = _ptr(bias)
    if bias is not None:
        _req(bias, F32, "bias")
    g.epi = epi
    if nchw_hw:
        _req(out, F32, "out")
        g.out_mode, g.hw = OUT_F32_NCHW, nchw_hw
        g.out, g.ldc = out.data_ptr(), 0
    else:
        f32out = out.dtype == F32
        _req(out, F32 if f32out else F16, "out", 16 if f32out else 8)
        r, c, ld = _rows(out, "out")
        if c != (2 * N_out if hilo_out else N_out):
            raise ValueError(f"out has {c} columns, expected {2 * N_out if hilo_out else N_out}")
        if hilo_out and f32out:
            raise ValueError("hilo_out writes fp16")
        g.out_mode, g.hw = (OUT_F16_HILO if hilo_out else OUT_F32_ROWMAJOR if f32out else OUT_F16_ROWMAJOR), 0
        g.out, g.ldc = out.data_ptr(), ld
        if out16 is not None:
            if not f32out:
                raise ValueError("out16 (fp16 copy) only goes with an fp32 out")
            _req(out16, F16, "out16", 8)
            r2, c2, ld2 = _rows(out16, "out16")
            if (r2, c2) != (r, c):
                raise ValueError("out16 shape mismatch")
            g.out2, g.ldc2 = out16.data_ptr(), ld2
    if res is not None:
        g.res_f32 = int(res.dtype == F32)
        _req(res, F32 if g.res_f32 else F16, "res", 16 if g.res_f32 else 8)
        g.res, g.ldres = res.data_ptr(), _rows(res, "res")[2]
    if gate is not None:
        _req(gate, F32, "gate", 4)
        g.gate = gate.data_ptr()
    if rowbias is not None:
        g.rowbias_f32 = int(rowbias.dtype == F32)
        _req(rowbias, F32 if g.rowbias_f32 else F16, "rowbias", 16 if g.rowbias_f32 else 8)
        g.rowbias, g.ld_rowbias, g.rows_per_sample = rowbias.data_ptr(), _rows(rowbias, "rowbias")[2], rows_per_sample


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias=None, epi: int = EPI_BIAS, res=None, gate=None,
         rowbias=None, rows_per_sample: int = 0, a2: Optional[torch.Tensor] = None, nchw_hw: int = 0, out16=None,
         vt: Optional[torch.Tensor] = None, vt_col0: int = 0, vt_rows: int = 0, hilo_a: bool = False, hilo_out: bool = False,
         wsplit: int = 0, vt_lo: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = [a | a2] @ w.T (+ epilogue).  a [M, K1], a2 [M, K2] (optional), w [N, K1+K2] fp16.
    ``hilo_a``: a is [M, 2K] = [hi | lo] of a split-fp16 activation and w [N, K] is used for both halves (gl_gemm_args.kwrap);
    ``hilo_out``: out is fp16 [M, 2N] = [hi | lo] of the result (GL_OUT_F16_HILO).
    ``wsplit``: w is [N, 2K] = [Whi | Wlo] rows of a split-fp16 weight: 1 = use Whi only (K or, with hilo_a, 2K products), 2 = with hilo_a the
    three-pass product xhi.Whi + xlo.Whi + xhi.Wlo (K index 3K; the third A segment is the hi half again, passed as the second source).
    ``vt`` [B, H, d, ldvt] fp16: columns [vt_col0, N) are written there as gl_attention's V^T operand (row m = sample
    m // vt_rows, key m % vt_rows) instead of to ``out`` (fused QKV projection)."""
    _req(a, F16, "a")
    _req(w, F16, "w")
    M, K1, lda = _rows(a, "a")
    N, K, ldw = _rows(w, "w")
    if ldw != K:
        raise ValueError("w must be contiguous")
    g = GemmArgs()
    g.a, g.lda = a.data_ptr(), lda
    if wsplit:
        if K % 2 or (wsplit == 2 and (not hilo_a or a2 is not None)):
            raise ValueError("wsplit: w must be [N, 2K]; the three-pass form needs hilo_a and no second source")
        K //= 2
        g.ldw = 2 * K
    if wsplit == 2:
        if K1 != 2 * K:
            raise ValueError(f"hilo_a: a has {K1} columns, expected 2 x K = {2 * K}")
        g.kwrap = K
        g.a2, g.lda2, g.ksplit = a.data_ptr(), lda, 2 * K
        K = 3 * K
    elif a2 is not None:
        _req(a2, F16, "a2")
        M2, K2, lda2 = _rows(a2, "a2")
        if M2 != M or K1 + K2 != K:
            raise ValueError("a2 shape mismatch")
        g.a2, g.lda2, g.ksplit = a2.data_ptr(), lda2, K1
    elif hilo_a:
        if K1 != 2 * K:
            raise ValueError(f"hilo_a: a has {K1} columns, expected 2 x K = {2 * K}")
        g.kwrap = K
        if not wsplit:
            g.ldw = K
        K = 2 * K
    elif K1 != K:
        raise ValueError(f"a has K={K1}, w has K={K}")
    g.w = w.data_ptr()
    g.M, g.N, g.K = M, N, K
    _fill_epilogue(g, epi, out, N // 2 if epi == EPI_GEGLU else N, bias, res, gate, rowbias, rows_per_sample, nchw_hw, out16, hilo_out)
    if vt is not None:
        _req(vt, F16, "vt")
        if vt.dim() != 4 or not vt.is_contiguous():
            raise ValueError("vt must be a contiguous [B, H, d, ldvt] tensor")
        g.vt, g.vt_col0, g.vt_rows = vt.data_ptr(), vt_col0, vt_rows
        g.vt_H, g.vt_d, g.vt_ld = vt.shape[1], vt.shape[2], vt.shape[3]
        if vt_lo is not None:              # ``hilo_out``: the fp16 residual of the V^T tail, same layout as ``vt`` (ABI 15)
            _req(vt_lo, F16, "vt_lo")
            if tuple(vt_lo.shape) != tuple(vt.shape) or not vt_lo.is_contiguous():
                raise ValueError("vt_lo must have vt's shape")
            g.vt_lo = vt_lo.data_ptr()
    check(_lib.lib().gl_gemm(C.byref(g), _stream()), "gl_gemm")
    return out


def conv3x3(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, B: int, Hin: int, Win: int, bias=None,
            stride: int = 1, upsample2x: bool = False, epi: int = EPI_BIAS, res=None, rowbias=None,
            rows_per_sample: int = 0, nchw_hw: int = 0, n_valid: Optional[int] = None, out16=None, in_split: int = 0,
            w_split: bool = False, pad01: bool = False) -> torch.Tensor:
    """x [B*Hin*Win, Cin] fp16 NHWC; w [Cout, 9*Cin] fp16 (tap-major, channel-minor).
    ``upsample2x`` with w [4*Cout, 4*Cin] (weights.pack_conv_upfold): the folded form of the layer (gl_conv_args.upsample2x = 2).
    ``pad01`` (stride 2): the VAE encoder's Downsample, F.pad(x, (0, 1, 0, 1)) + pad-0 conv (gl_conv3x3_pad01), Hout = Hin // 2.
    ``in_split`` = 2: x is [B*Hin*Win, 2 Cin] = [hi | lo] pixel rows of a split-fp16 activation, both halves against the same weight;
    3 (with ``w_split``): plus the third pass hi.Wlo.  ``w_split``: w is [Cout, 18 Cin] = rows [Whi | Wlo] (gl_conv_args)."""
    _req(x, F16, "x")
    _req(w, F16, "w")
    rows, Cin, ldx = _rows(x, "x")
    if ldx != Cin or rows != B * Hin * Win:
        raise ValueError("x must be a contiguous [B*Hin*Win, Cin] matrix")
    if in_split:
        Cin //= 2
    N, K, _ = _rows(w, "w")
    folded = bool(upsample2x) and K == 4 * Cin and not w_split
    if folded:
        if n_valid is not None:         # the kernel finds parity p's rows at p * g.N: g.N must be the packed Cout
            raise ValueError("n_valid does not go with folded upsample weights")
        if N % 4:
            raise ValueError("folded upsample weights must be [4*Cout, 4*Cin]")
        N //= 4
    elif K != (18 if w_split else 9) * Cin:
        raise ValueError("w must be [Cout, 9*Cin] ([Cout, 18*Cin] with w_split; [4*Cout, 4*Cin] folded upsample weights)")
    if upsample2x:
        Hout, Wout = 2 * Hin, 2 * Win
    elif pad01:
        Hout, Wout = Hin // 2, Win // 2
    else:
        Hout, Wout = (Hin + 2 - 3) // stride + 1, (Win + 2 - 3) // stride + 1
    a = ConvArgs()
    a.inp = x.data_ptr()
    a.B, a.Hin, a.Win, a.Cin, a.Hout, a.Wout = B, Hin, Win, Cin, Hout, Wout
    a.stride, a.upsample2x = stride, (2 if folded else int(bool(upsample2x)))
    a.in_split, a.w_split = int(in_split), int(bool(w_split))
    a.g.w = w.data_ptr()
    a.g.N = N if n_valid is None else n_valid
    _fill_epilogue(a.g, epi, out, a.g.N, bias, res, None, rowbias, rows_per_sample, nchw_hw, out16)
    if pad01:
        check(_lib.lib().gl_conv3x3_pad01(C.byref(a), _stream()), "gl_conv3x3_pad01")
    else:
        check(_lib.lib().gl_conv3x3(C.byref(a), _stream()), "gl_conv3x3")
    return out


def conv3x3_pad01(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, B: int, Hin: int, Win: int, bias=None, **kw) -> torch.Tensor:
    """conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) on NHWC fp16 x (model.py:60-79): output [B*(Hin//2)*(Win//2), Cout]."""
    return conv3x3(x, w, out, B, Hin, Win, bias, stride=2, pad01=True, **kw)


def vt_ld(Nk: int) -> int:
    """Row stride (keys) for a V^T buffer: Nk rounded up to the 64-key tile, plus one tile when that is a multiple of
    512 keys -- a 1 KiB-multiple row stride maps the d rows of every V^T tile onto the same L1 sets / channels
    (measured 307 vs 277 us at N = 4096, d = 40)."""
    n = (Nk + 63) // 64 * 64
    return n + 64 if n % 512 == 0 else n


def transpose_v(v: torch.Tensor, v_bstride: int, ldv: int, vt: torch.Tensor, B: int, H: int, d: int, Nk: int):
    """v: fp16 view whose element (b, key, h*d + c) sits at v.data_ptr + b*v_bstride + key*ldv + h*d + c.
    vt: [B, H, d, ldvt] fp16 contiguous, ldvt >= roundup(Nk, 64)."""
    _req(v, F16, "v", 2)
    _req(vt, F16, "vt")
    ldvt = vt.shape[-1]
    check(_lib.lib().gl_transpose_v(v.data_ptr(), v_bstride, ldv, vt.data_ptr(), ldvt, B, H, d, Nk, _stream()),
          "gl_transpose_v")
    return vt


def attention(q: torch.Tensor, q_bstride: int, ldq: int, k: torch.Tensor, k_bstride: int, ldk: int, vt: torch.Tensor,
              out: torch.Tensor, o_bstride: int, ldo: int, B: int, H: int, d: int, Nq: int, Nk: int, scale: float,
              q_prescaled: bool = False, q_lo=None, k_lo=None, vt_lo=None, out_lo=None):
    """``q_prescaled``: scale * log2(e) is already folded into q (weights.Q_FOLD does that to the packed q projections).
    ``q_lo`` / ``k_lo`` / ``vt_lo`` (all three, same layouts as q / k / vt): the fp16 residuals of split-fp16 operands -> the three-pass
    split attention kernel; ``out_lo`` then receives fp16(O - fp16(O))."""
    _req(q, F16, "q")
    _req(k, F16, "k")
    _req(vt, F16, "vt")
    _req(out, F16, "out", 8)
    a = AttnArgs()
    a.q, a.q_bstride, a.ldq = q.data_ptr(), q_bstride, ldq
    a.k, a.k_bstride, a.ldk = k.data_ptr(), k_bstride, ldk
    a.vt, a.ldvt = vt.data_ptr(), vt.shape[-1]
    a.out, a.o_bstride, a.ldo = out.data_ptr(), o_bstride, ldo
    a.B, a.H, a.d, a.Nq, a.Nk = B, H, d, Nq, Nk
    a.scale = scale
    a.q_prescaled = int(q_prescaled)
    for t_, n_ in ((q_lo, "q_lo"), (k_lo, "k_lo"), (vt_lo, "vt_lo"), (out_lo, "out_lo")):
        if t_ is not None:
            _req(t_, F16, n_, 8)
    a.q_lo, a.k_lo, a.vt_lo, a.out_lo = _ptr(q_lo), _ptr(k_lo), _ptr(vt_lo), _ptr(out_lo)
    check(_lib.lib().gl_attention(C.byref(a), _stream()), "gl_attention")
    return out


def gn_nchunk(HW: int) -> int:
    """pixel chunks per sample for the GroupNorm partial sums: 64 for the UNet's maps (<= 64x64), more for the
    VAE decoder's large maps so the statistics pass still fills the chip"""
    if HW <= 4096:
        return max(1, min(64, HW // 4))
    return min(512, HW // 512)


def groupnorm(x1: torch.Tensor, x2: Optional[torch.Tensor], B: int, HW: int, gamma: torch.Tensor, beta: torch.Tensor,
              eps: float, silu: bool, out: torch.Tensor, partial: torch.Tensor, out_lo: Optional[torch.Tensor] = None,
              raw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm(32) of the channel concat [x1 | x2] (x2 may be None); x* are [B*HW, C*], both fp16 or both fp32 (the residual
    stream).  ``out`` fp16 [B*HW, C] (may be a column view of a wider buffer); ``out_lo`` (optional, same row stride): the
    fp16 residual of the normalised rows; ``raw`` (optional) fp16 [B*HW, >= 2C]: the INPUT as [hi | lo] (gl_groupnorm_ex)."""
    xf32 = x1.dtype == F32
    _req(x1, F32 if xf32 else F16, "x1")
    C1 = x1.shape[-1]
    C2 = 0
    if x2 is not None:
        _req(x2, F32 if xf32 else F16, "x2")
        C2 = x2.shape[-1]
    _req(gamma, F32, "gamma")
    _req(beta, F32, "beta")
    for t_, n_ in ((out, "out"), (out_lo, "out_lo"), (raw, "raw")):
        if t_ is not None and (t_.dtype != F16 or not t_.is_cuda or t_.stride(-1) != 1 or t_.data_ptr() % 16):
            raise _lib.HipLibraryError(f"{n_}: fp16 GPU rows, 16-byte aligned")
    _req(partial, F32, "partial")
    nchunk = gn_nchunk(HW)
    if partial.numel() < B * nchunk * 64:
        raise ValueError("partial buffer too small")
    a = GnArgs()
    a.x1, a.C1, a.x2, a.C2, a.x_f32, a.B, a.HW = x1.data_ptr(), C1, _ptr(x2), C2, int(xf32), B, HW
    a.gamma, a.beta, a.eps, a.silu = gamma.data_ptr(), beta.data_ptr(), eps, int(silu)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    if out_lo is not None:
        if out_lo.stride(0) != out.stride(0):
            raise ValueError("out_lo must have out's row stride")
        a.out_lo = out_lo.data_ptr()
    if raw is not None:
        a.raw, a.ldraw = raw.data_ptr(), raw.stride(0)
    a.partial, a.nchunk = partial.data_ptr(), nchunk
    check(_lib.lib().gl_groupnorm_ex(C.byref(a), _stream()), "gl_groupnorm_ex")
    return out


def layernorm(x: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, B: int, rows_in: int,
              rows_out: Optional[int] = None, row_off: int = 0, eps: float = 1e-5, stats: Optional[torch.Tensor] = None,
              x2: Optional[torch.Tensor] = None, rows2: int = 0, y_lo: bool = False) -> torch.Tensor:
    """``y_lo``: y is fp16 [B*rows_out, >= 2C] and receives [hi | lo] rows (gl_layernorm x_f32 bit 3; fp32 inputs only).
    x [B*rows_in, C] fp16 or fp32 (residual stream) -> y fp16 (or fp32: the dtype of ``y`` decides) rows b*rows_out + row_off + i (y is [B*rows_out, C]);
    ``stats`` (optional fp32 [B*rows_in, 2]) receives (mean, rstd) per row.  ``x2`` (fp16 [B*rows2, C]): a second source
    whose rows follow x's rows inside every sample's block of y ([x ; objs] in one launch)."""
    xf32 = x.dtype == F32
    yf32 = y.dtype == F32
    _req(x, F32 if xf32 else F16, "x")
    _req(y, F32 if yf32 else F16, "y")
    _req(gamma, F32, "gamma")
    _req(beta, F32, "beta")
    _, Cc, ldx = _rows(x, "x")
    _, _, ldy = _rows(y, "y")
    rows_out = rows_in if rows_out is None else rows_out
    if stats is not None:
        _req(stats, F32, "stats", 8)
        if stats.numel() < 2 * B * rows_in:
            raise ValueError("stats buffer too small")
    ldx2 = 0
    x2f32 = False
    if x2 is not None:
        x2f32 = x2.dtype == F32
        _req(x2, F32 if x2f32 else F16, "x2")
        ldx2 = _rows(x2, "x2")[2]
    check(_lib.lib().gl_layernorm(x.data_ptr(), ldx, int(xf32) | (2 if yf32 else 0) | (4 if x2f32 else 0) | (8 if y_lo else 0), y.data_ptr(), ldy, gamma.data_ptr(), beta.data_ptr(), B, rows_in,
                                  rows_out, row_off, Cc, eps, _ptr(stats), _ptr(x2), ldx2, rows2, _stream()), "gl_layernorm")
    return y


def rela_pool(hid, B, H, W, Cc, rects, nvalid, poison, max_objs, feat, ln_gamma=None, ln_beta=None, ln_out=None, slots=0):
    """feat[b, i] = mean of hid over box i; with ``ln_out`` also LayerNorm(feat) (fused norm1 of rela_fuse).  ``slots``: rows per sample of
    feat / ln_out (0 = max_objs; every nvalid[b] must be <= slots)."""
    _req(hid, F16, "hid")
    _req(feat, F16, "feat")
    for t, n in ((rects, "rects"), (nvalid, "nvalid"), (poison, "poison")):
        _req(t, torch.int32, n, 4)
    if ln_out is not None:
        _req(ln_out, F16, "ln_out")
        _req(ln_gamma, F32, "ln_gamma")
        _req(ln_beta, F32, "ln_beta")
    check(_lib.lib().gl_rela_pool(hid.data_ptr(), B, H, W, Cc, rects.data_ptr(), nvalid.data_ptr(), poison.data_ptr(),
                                  max_objs, int(slots), feat.data_ptr(), _ptr(ln_gamma), _ptr(ln_beta), _ptr(ln_out), _stream()), "gl_rela_pool")
    return feat


def split_f32(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """fp32 rows [rows, C] -> fp16 [rows, 2C] = [hi | lo] (gl_split_f32)."""
    _req(x, F32, "x")
    _req(y, F16, "y")
    rows, Cc, ldx = _rows(x, "x")
    _, c2, ldy = _rows(y, "y")
    if c2 != 2 * Cc:
        raise ValueError("y must be [rows, 2C]")
    check(_lib.lib().gl_split_f32(x.data_ptr(), ldx, rows, Cc, y.data_ptr(), ldy, _stream()), "gl_split_f32")
    return y


def layernorm_stats(x: torch.Tensor, stats: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """per-row (mean, rstd) of fp32 rows [rows, C] -> stats fp32 [rows, 2] (gl_layernorm_stats: gl_layernorm's statistics alone)."""
    _req(x, F32, "x")
    _req(stats, F32, "stats", 8)
    rows, Cc, ldx = _rows(x, "x")
    if stats.numel() < 2 * rows:
        raise ValueError("stats buffer too small")
    check(_lib.lib().gl_layernorm_stats(x.data_ptr(), ldx, rows, Cc, eps, stats.data_ptr(), _stream()), "gl_layernorm_stats")
    return stats


def rela_pool_ln3(x, ln3_stats, ln3_gamma, ln3_beta, B, H, W, Cc, rects, nvalid, poison, max_objs, feat, ln_gamma=None, ln_beta=None, ln_out=None, slots=0):
    """rela_pool on the fp32 stream: feat[b, i] = mean over box i of LN3(x), LN3 re-evaluated in fp32 from ``ln3_stats`` (gl_rela_pool_ln3)."""
    _req(x, F32, "x")
    _req(ln3_stats, F32, "ln3_stats", 8)
    _req(ln3_gamma, F32, "ln3_gamma")
    _req(ln3_beta, F32, "ln3_beta")
    _req(feat, F16, "feat")
    for t, n in ((rects, "rects"), (nvalid, "nvalid"), (poison, "poison")):
        _req(t, torch.int32, n, 4)
    if ln_out is not None:
        _req(ln_out, F16, "ln_out")
        _req(ln_gamma, F32, "ln_gamma")
        _req(ln_beta, F32, "ln_beta")
    check(_lib.lib().gl_rela_pool_ln3(x.data_ptr(), ln3_stats.data_ptr(), ln3_gamma.data_ptr(), ln3_beta.data_ptr(), B, H, W, Cc, rects.data_ptr(),
                                      nvalid.data_ptr(), poison.data_ptr(), max_objs, int(slots), feat.data_ptr(), _ptr(ln_gamma), _ptr(ln_beta), _ptr(ln_out),
                                      _stream()), "gl_rela_pool_ln3")
    return feat


def rela_merge(x, hid, f, B, H, W, Cc, rects, nvalid, poison, max_objs, y, ln_stats=None, gamma=None, beta=None,
               ln2_gamma=None, ln2_beta=None, ln2_out=None, slots=0):
    """y = 0.5 * (x + hid + (1/max_objs) sum_i 1[p in rect_i] f_i); x / y fp16 or fp32 (same dtype).  With ``ln_stats``
    (+ gamma, beta) hid = LayerNorm(x) is re-evaluated in fp32 from the stored (mean, rstd) instead of read from ``hid``.
    With ``ln2_out`` (fp32 stream + ln_stats form) the launch also writes LayerNorm(y; ln2_gamma, ln2_beta) in fp16."""
    xf32 = x.dtype == F32
    for t, n in ((x, "x"), (y, "y")):
        _req(t, F32 if xf32 else F16, n)
    _req(f, F16, "f")
    if ln_stats is None:
        _req(hid, F16, "hid")
    else:
        for t, n in ((ln_stats, "ln_stats"), (gamma, "gamma"), (beta, "beta")):
            _req(t, F32, n, 8)
    if ln2_out is not None:
        _req(ln2_out, F16, "ln2_out")
        for t, n in ((ln2_gamma, "ln2_gamma"), (ln2_beta, "ln2_beta")):
            _req(t, F32, n, 8)
    check(_lib.lib().gl_rela_merge(x.data_ptr(), int(xf32), _ptr(hid), _ptr(ln_stats), _ptr(gamma), _ptr(beta), f.data_ptr(), B, H, W,
                                   Cc, rects.data_ptr(), nvalid.data_ptr(), poison.data_ptr(), max_objs, int(slots), y.data_ptr(), _ptr(ln2_gamma),
                                   _ptr(ln2_beta), _ptr(ln2_out), _stream()),
          "gl_rela_merge")
    return y


def ff_fused_supported(Cc: int) -> bool:
    return bool(_lib.lib().gl_ff_fused_supported(int(Cc)))


def ff_fused_applicable(Cc: int, M: int) -> bool:
    """the engine's own rule for taking the fused FeedForward (gl_ff_fused_applicable)"""
    return bool(_lib.lib().gl_ff_fused_applicable(int(Cc), int(M)))


def ff_fused(x, w1, b1, w2, b2, res, out, gate=None, hilo_out: bool = False):
    """out = res (+ | gate *) (GEGLU(x . w1^T + b1) . w2^T + b2) in one launch (gl_ff_fused; attention.py:38-62).
    x fp16 [M, C]; w1 / b1 the packed GEGLU operands [8C, C] / [8C]; w2 [C, 4C]; res fp32 or fp16 [M, C]; out fp16 or fp32."""
    _req(x, F16, "x")
    _req(w1, F16, "w1")
    _req(w2, F16, "w2")
    _req(b1, F32, "b1")
    _req(b2, F32, "b2")
    M, Cc = x.shape
    if w1.shape != (8 * Cc, Cc) or w2.shape != (Cc, 4 * Cc) or not w1.is_contiguous() or not w2.is_contiguous():
        raise ValueError("w1 must be [8C, C] (packed GEGLU layout) and w2 [C, 4C], contiguous")
    if res.dtype not in (F16, F32) or out.dtype not in (F16, F32) or not res.is_cuda or not out.is_cuda:
        raise _lib.HipLibraryError("res / out: fp16 or fp32 GPU tensors")
    a = _lib.FFArgs()
    a.x, a.ldx = x.data_ptr(), x.stride(0)
    a.w1, a.b1, a.w2, a.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    a.res, a.ldres, a.res_f32 = res.data_ptr(), res.stride(0), int(res.dtype == F32)
    a.gate = _ptr(gate)
    a.out, a.ldc, a.out_mode = out.data_ptr(), out.stride(0), (OUT_F16_HILO if hilo_out else OUT_F32_ROWMAJOR if out.dtype == F32 else OUT_F16_ROWMAJOR)
    a.M, a.C = M, Cc
    check(_lib.lib().gl_ff_fused(C.byref(a), _stream()), "gl_ff_fused")
    return out


def posnet_input(boxes, masks, emb, null_pos, null_xyxy, num_freqs, out):
    for t, n in ((boxes, "boxes"), (masks, "masks"), (emb, "emb"), (null_pos, "null_pos"), (null_xyxy, "null_xyxy")):
        _req(t, F32, n, 4)
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    _req(out, F16, "out")
    rows = boxes.shape[0] * boxes.shape[1]
    in_dim = emb.shape[-1]
    check(_lib.lib().gl_posnet_input(boxes.data_ptr(), masks.data_ptr(), emb.data_ptr(), null_pos.data_ptr(),
                                     null_xyxy.data_ptr(), rows, in_dim, num_freqs, out.data_ptr(), _stream()),
          "gl_posnet_input")
    return out


def posnet_input_kp(points, masks, person_emb, keypoint_emb, null_person, null_xy, num_freqs, out):
    """The MLP input of the keypoint PositionNet (gl_posnet_input_kp / _f32 by ``out``'s dtype): points [B, 17 P, 2], masks [B, 17 P],
    person_emb [P, D], keypoint_emb [17, D], null_person [D], null_xy [4 * num_freqs], fp32; out [B, 17 P, ld] fp16 or fp32 with
    ld = D + 4 * num_freqs rounded up to a multiple of 64 (the kernel writes the pad columns as zeros)."""
    for t, n in ((points, "points"), (masks, "masks"), (person_emb, "person_emb"), (keypoint_emb, "keypoint_emb"), (null_person, "null_person"),
                 (null_xy, "null_xy")):
        _req(t, F32, n, 4)
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    if points.dim() != 3 or points.shape[2] != 2 or person_emb.dim() != 2 or keypoint_emb.dim() != 2:
        raise ValueError("posnet_input_kp: points [B, 17 P, 2], person_emb [P, D], keypoint_emb [17, D]")
    B, tokens = points.shape[0], points.shape[1]
    P, D = person_emb.shape
    if tokens != 17 * P or tuple(masks.shape) != (B, tokens) or tuple(keypoint_emb.shape) != (17, D) or null_person.numel() != D or \
            null_xy.numel() != 4 * num_freqs:
        raise ValueError("posnet_input_kp: inconsistent shapes")
    ld = (D + 4 * num_freqs + 63) // 64 * 64
    _req(out, F32 if out.dtype == F32 else F16, "out", 4)
    if not out.is_contiguous() or out.numel() != B * tokens * ld:
        raise ValueError(f"out: need a contiguous [B, 17 P, {ld}] tensor")
    fn = _lib.lib().gl_posnet_input_kp_f32 if out.dtype == F32 else _lib.lib().gl_posnet_input_kp
    check(fn(points.data_ptr(), masks.data_ptr(), person_emb.data_ptr(), keypoint_emb.data_ptr(), null_person.data_ptr(), null_xy.data_ptr(),
             B, tokens, D, num_freqs, out.data_ptr(), _stream()), "gl_posnet_input_kp")
    return out


def posnet_input_ti(boxes, masks, text_masks, image_masks, text_emb, image_emb, null_text, null_image, null_xyxy, num_freqs, out_text, out_image):
    """Both MLP inputs of the text_image PositionNet (gl_posnet_input_ti / _f32 by the outputs' dtype): out_text / out_image
    [B, n, in_dim + 8 * num_freqs], both fp16 or both fp32."""
    for t, n in ((boxes, "boxes"), (masks, "masks"), (text_masks, "text_masks"), (image_masks, "image_masks"), (text_emb, "text_emb"),
                 (image_emb, "image_emb"), (null_text, "null_text"), (null_image, "null_image"), (null_xyxy, "null_xyxy")):
        _req(t, F32, n, 4)
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    rows, in_dim = boxes.shape[0] * boxes.shape[1], text_emb.shape[-1]
    if masks.numel() != rows or text_masks.numel() != rows or image_masks.numel() != rows or text_emb.numel() != rows * in_dim or \
            image_emb.shape != text_emb.shape or null_text.numel() != in_dim or null_image.numel() != in_dim or null_xyxy.numel() != 8 * num_freqs:
        raise ValueError("posnet_input_ti: inconsistent shapes")
    f32out = out_text.dtype == F32
    for o, n in ((out_text, "out_text"), (out_image, "out_image")):
        _req(o, F32 if f32out else F16, n, 4)
        if not o.is_contiguous() or o.numel() != rows * (in_dim + 8 * num_freqs):
            raise ValueError(f"{n}: need a contiguous [rows, in_dim + 8 * num_freqs] tensor")
    fn = _lib.lib().gl_posnet_input_ti_f32 if f32out else _lib.lib().gl_posnet_input_ti
    check(fn(boxes.data_ptr(), masks.data_ptr(), text_masks.data_ptr(), image_masks.data_ptr(), text_emb.data_ptr(), image_emb.data_ptr(),
             null_text.data_ptr(), null_image.data_ptr(), null_xyxy.data_ptr(), rows, in_dim, num_freqs, out_text.data_ptr(), out_image.data_ptr(),
             _stream()), "gl_posnet_input_ti")
    return out_text, out_image


def image_ground_feature(feat: torch.Tensor, proj: torch.Tensor, norm: float = 28.7, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = norm * (feat[i] @ proj) / ||feat[i] @ proj||_2 in fp32 (interface.py:126-129): feat [n, dim], proj [dim, dim], dim <= 1024."""
    _req(feat, F32, "feat", 4)
    _req(proj, F32, "proj", 4)
    if feat.dim() != 2 or tuple(proj.shape) != (feat.shape[1], feat.shape[1]) or not feat.is_contiguous() or not proj.is_contiguous():
        raise ValueError("image_ground_feature: feat [n, dim] and proj [dim, dim], contiguous")
    if feat.shape[1] > 1024:
        raise ValueError("image_ground_feature: dim <= 1024")
    if out is None:
        out = torch.empty_like(feat)
    _req(out, F32, "out", 4)
    if out.shape != feat.shape or not out.is_contiguous():
        raise ValueError("image_ground_feature: out must be contiguous with feat's shape")
    check(_lib.lib().gl_image_ground_feature(feat.data_ptr(), proj.data_ptr(), feat.shape[0], feat.shape[1], float(norm), out.data_ptr(), _stream()),
          "gl_image_ground_feature")
    return out


def timestep_embedding(t: torch.Tensor, dim: int, out: torch.Tensor):
    _req(t, F32, "t", 4)
    _req(out, F16, "out")
    check(_lib.lib().gl_timestep_embedding(t.data_ptr(), t.shape[0], dim, out.data_ptr(), _stream()),
          "gl_timestep_embedding")
    return out


def silu(x: torch.Tensor, y: torch.Tensor):
    _req(x, F16, "x")
    _req(y, F16, "y")
    check(_lib.lib().gl_silu_f16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "gl_silu_f16")
    return y


def cfg_combine(eps2b: torch.Tensor, guidance: float, e_out: torch.Tensor):
    _req(eps2b, F32, "eps2b")
    _req(e_out, F32, "e_out")
    check(_lib.lib().gl_cfg_combine(eps2b.data_ptr(), guidance, e_out.numel(), e_out.data_ptr(), _stream()),
          "gl_cfg_combine")
    return e_out


def cfg3_combine(eps3b: torch.Tensor, s_text: float, s_layout: float, e_out: torch.Tensor):
    """Guidance with separate text and layout scales (gl_cfg3_combine): ``eps3b`` = the UNet output of the [cond ; text-only ; uncond] batch,
    three times ``e_out``'s elements; e_out = (e_u + s_text * (e_t - e_u)) + s_layout * (e_c - e_t), bit-identical to that torch fp32
    expression.  ``e_out`` must not overlap ``eps3b``."""
    for t, nm in ((eps3b, "eps3b"), (e_out, "e_out")):
        _req(t, F32, nm, 4)
        if not t.is_contiguous():
            raise ValueError(f"{nm}: need a contiguous tensor")
    n = e_out.numel()
    if n == 0 or eps3b.numel() != 3 * n:
        raise ValueError(f"eps3b {tuple(eps3b.shape)}: need three times e_out's {tuple(e_out.shape)} elements ([cond ; text-only ; uncond])")
    check(_lib.lib().gl_cfg3_combine(eps3b.data_ptr(), float(s_text), float(s_layout), n, e_out.data_ptr(), _stream()), "gl_cfg3_combine")
    return e_out


def plms_update(x, e, olds, coefs, div, sqrt_at, s1m, sqrt_aprev, dir_coef, x_prev):
    """x_prev from e' = (coefs[0]*e + sum coefs[1+j]*olds[j]) / div (plms.py:144-161)."""
    _req(x, F32, "x")
    _req(e, F32, "e")
    _req(x_prev, F32, "x_prev")
    ps = [None, None, None]
    cs = [0.0, 0.0, 0.0]
    for j, o in enumerate(olds):
        _req(o, F32, "old_eps")
        ps[j] = o.data_ptr()
        cs[j] = float(coefs[1 + j])
    check(_lib.lib().gl_plms_update(x.data_ptr(), e.data_ptr(), ps[0], ps[1], ps[2], float(coefs[0]), cs[0], cs[1],
                                    cs[2], float(div), float(sqrt_at), float(s1m), float(sqrt_aprev), float(dir_coef),
                                    x.numel(), x_prev.data_ptr(), _stream()), "gl_plms_update")
    return x_prev


def _update_operands(eps, x, more, required=()) -> int:
    """The operands of a fused sampler update (ddim_update, dpmpp_update): ``eps``, ``x`` and the (name, tensor) pairs of ``more`` are
    contiguous fp32 GPU tensors, 4-byte aligned; None passes unless the name is in ``required``; eps holds x's elements once or twice, every
    other operand once.  Returns x's element count."""
    for nm, t in [("eps", eps), ("x", x), *more]:
        if t is None:
            if nm in required:
                raise ValueError(f"{nm}: required")
            continue
        _req(t, F32, nm, 4)
        if not t.is_contiguous():
            raise ValueError(f"{nm}: need a contiguous tensor")
    n = x.numel()
    if n == 0 or eps.numel() not in (n, 2 * n):
        raise ValueError(f"eps {tuple(eps.shape)}: need x's {tuple(x.shape)} elements once, or twice ([cond ; uncond])")
    for nm, t in more:
        if t is not None and t.numel() != n:
            raise ValueError(f"{nm} {tuple(t.shape)}: need x's shape {tuple(x.shape)}")
    return n


def ddim_update(eps: torch.Tensor, x: torch.Tensor, x_out: torch.Tensor, *, sqrt_at: float, s1m: float, sqrt_aprev: float, dir_coef: float,
                sigma: float = 0.0, noise: Optional[torch.Tensor] = None, guidance: float = 1.0, pred_x0: Optional[torch.Tensor] = None):
    """One DDIM update in one launch (gl_ddim_update, ddim.py:115-135).  ``eps``: the UNet output, x's shape, or twice x's batch = the
    [cond ; uncond] halves, combined with ``guidance`` inside the launch.  ``x_out`` may be ``x``; ``noise`` None = the reference's
    ``0 * randn`` (the term is skipped); ``pred_x0`` optionally receives the x0 prediction.  Bit-identical to the torch fp32 expression."""
    n = _update_operands(eps, x, [("x_out", x_out), ("noise", noise), ("pred_x0", pred_x0)])
    check(_lib.lib().gl_ddim_update(eps.data_ptr(), x.data_ptr(), _ptr(noise), eps.numel() // n, float(guidance), float(sqrt_at), float(s1m),
                                    float(sqrt_aprev), float(dir_coef), float(sigma), n, x_out.data_ptr(), _ptr(pred_x0), _stream()),
          "gl_ddim_update")
    return x_out


def dpmpp_update(eps: torch.Tensor, x: torch.Tensor, x_out: torch.Tensor, x0_out: torch.Tensor, *, sqrt_at: float, s1m: float, c_x: float,
                 c_d: float, w1: float = 1.0, w0: float = 0.0, x0_old: Optional[torch.Tensor] = None, guidance: float = 1.0):
    """One DPM-Solver++(2M) update in one launch (gl_dpmpp_update): x0 = (x - s1m * e) / sqrt_at, D = w1 * x0 + w0 * x0_old,
    x_out = c_x * x + c_d * D (host.dpm_step_coefs).  ``eps``: the UNet output, x's shape, or twice x's batch = the [cond ; uncond] halves,
    combined with ``guidance`` inside the launch.  ``x0_old`` None = a first-order step (``w0`` must be 0).  ``x0_out`` receives x0, the
    history of the next step; ``x_out`` may be ``x`` and ``x0_out`` may be ``x0_old``.  Bit-identical to the torch fp32 expression."""
    n = _update_operands(eps, x, [("x_out", x_out), ("x0_out", x0_out), ("x0_old", x0_old)], required=("eps", "x", "x_out", "x0_out"))
    if x0_old is None and w0 != 0:
        raise ValueError(f"w0 = {w0} without x0_old: a first-order step has no history term")
    check(_lib.lib().gl_dpmpp_update(eps.data_ptr(), x.data_ptr(), _ptr(x0_old), eps.numel() // n, float(guidance), float(sqrt_at), float(s1m),
                                     float(c_x), float(c_d), float(w1), float(w0), n, x_out.data_ptr(), x0_out.data_ptr(), _stream()),
          "gl_dpmpp_update")
    return x_out


def pack_latent(x: torch.Tensor, Cpad: int, reps: int, out: torch.Tensor, split: bool = False):
    """x fp32 [B, C, h, w] -> out fp16 [reps*B, h*w, Cpad]; ``split``: channels [hi | lo | hi] of x (first-conv weights [Whi | Whi | Wlo])."""
    _req(x, F32, "x")
    _req(out, F16, "out")
    B, Cc, h, w = x.shape
    check(_lib.lib().gl_pack_latent(x.data_ptr(), B, Cc, h * w, Cpad, reps, int(split), out.data_ptr(), _stream()), "gl_pack_latent")
    return out


def pack_latent_extra(x: torch.Tensor, extra: torch.Tensor, Cpad: int, reps: int, out: torch.Tensor, split: bool = False):
    """x fp32 [B, C, h, w] and extra fp32 [1|B, Ce, h, w] -> out fp16 [reps*B, h*w, Cpad] over cat([x, extra], dim=1) (the first-conv input of an
    inpaint_mode UNet); ``split``: channels [hi | lo | hi] of the C + Ce concatenated ones."""
    _req(x, F32, "x")
    _req(extra, F32, "extra")
    _req(out, F16, "out")
    B, Cc, h, w = x.shape
    if extra.dim() != 4 or tuple(extra.shape[-2:]) != (h, w) or extra.shape[0] not in (1, B):
        raise ValueError(f"extra {tuple(extra.shape)} does not go with x {tuple(x.shape)}")
    if out.numel() < reps * B * h * w * Cpad:
        raise ValueError("out is too small")
    check(_lib.lib().gl_pack_latent_extra(x.data_ptr(), extra.data_ptr(), B, extra.shape[0], Cc, extra.shape[1], h * w, Cpad, reps, int(split),
                                          out.data_ptr(), _stream()), "gl_pack_latent_extra")
    return out


def vae_posterior(h: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, noise: torch.Tensor, scale: float, z: torch.Tensor,
                  mean: Optional[torch.Tensor] = None) -> torch.Tensor:
    """h fp32 [B, Cin, h, w] (Encoder.conv_out) -> z fp32 [B, E, h, w] = (mean + exp(clamp(logvar, -30, 20) / 2) * noise) * scale with
    [mean | logvar] = quant_conv(h) in fp32 (w [2E, Cin], bias [2E]); ``mean`` optionally receives the posterior mean."""
    for t, n in ((h, "h"), (w, "w"), (bias, "bias"), (noise, "noise"), (z, "z")):
        _req(t, F32, n, 4)
    B, Cin, hh, ww = h.shape
    E = w.shape[0] // 2
    if w.shape != (2 * E, Cin) or tuple(z.shape) != (B, E, hh, ww) or noise.shape != z.shape:
        raise ValueError("vae_posterior: w [2E, Cin], noise / z [B, E, h, w]")
    if mean is not None:
        _req(mean, F32, "mean", 4)
    check(_lib.lib().gl_vae_posterior(h.data_ptr(), w.data_ptr(), bias.data_ptr(), noise.data_ptr(), float(scale), B, Cin, E, hh * ww,
                                      z.data_ptr(), _ptr(mean), _stream()), "gl_vae_posterior")
    return z


def latent_blend(x: torch.Tensor, x0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, a: float, s: float) -> torch.Tensor:
    """In place: x = (a * x0 + s * noise) * mask + (1 - mask) * x, bit-identical to that torch expression (plms.py:95-99).
    x fp32 [B, C, h, w]; x0 / noise [1|B, C, h, w]; mask [1|B, 1, h, w]."""
    for t, n in ((x, "x"), (x0, "x0"), (noise, "noise"), (mask, "mask")):
        _req(t, F32, n, 4)
    B, Cc, hh, ww = x.shape
    if x0.shape[1:] != x.shape[1:] or noise.shape != x0.shape or x0.shape[0] not in (1, B) or \
            tuple(mask.shape[1:]) != (1, hh, ww) or mask.shape[0] not in (1, B):
        raise ValueError("latent_blend: x0 / noise [1|B, C, h, w], mask [1|B, 1, h, w]")
    check(_lib.lib().gl_latent_blend(x.data_ptr(), x0.data_ptr(), noise.data_ptr(), mask.data_ptr(), float(a), float(s), B, Cc, hh * ww,
                                     x0.shape[0], mask.shape[0], _stream()), "gl_latent_blend")
    return x


def q_sample(x0: torch.Tensor, noise: torch.Tensor, a: float, s: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a * x0 + s * noise (gl_q_sample; ldm.py:19-22), bit-identical to that torch fp32 expression.  noise fp32 [B, C, h, w];
    x0 [1|B, C, h, w] (one image is broadcast over the batch); ``out`` [B, C, h, w]: None = a new tensor, may be ``noise`` (in place),
    must not overlap ``x0``."""
    if out is None:
        out = torch.empty_like(noise)
    for t, n in ((x0, "x0"), (noise, "noise"), (out, "out")):
        _req(t, F32, n, 4)
        if not t.is_contiguous():
            raise ValueError(f"{n}: need a contiguous tensor")
    if noise.dim() != 4 or noise.numel() == 0 or x0.shape[1:] != noise.shape[1:] or x0.shape[0] not in (1, noise.shape[0]) or out.shape != noise.shape:
        raise ValueError(f"q_sample: noise / out [B, C, h, w], x0 [1|B, C, h, w], got x0 {tuple(x0.shape)}, noise {tuple(noise.shape)}, "
                         f"out {tuple(out.shape)}")
    B, Cc, hh, ww = noise.shape
    check(_lib.lib().gl_q_sample(x0.data_ptr(), noise.data_ptr(), float(a), float(s), B, Cc * hh * ww, x0.shape[0], out.data_ptr(), _stream()),
          "gl_q_sample")
    return out


def softmax_rows(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """in-place softmax(scale * x) over the last dim of a 2-D fp16 tensor"""
    _req(x, F16, "x")
    rows, n, ld = _rows(x, "x")
    check(_lib.lib().gl_softmax_rows(x.data_ptr(), rows, n, ld, scale, _stream()), "gl_softmax_rows")
    return x


def latent_affine_pack(z: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, pre: float, Cpad: int, out: torch.Tensor):
    """z fp32 [B, C, h, w] -> out fp16 [B*h*w, Cpad] = post_quant_conv(z * pre), zero-padded channels"""
    for t, n in ((z, "z"), (w, "w"), (bias, "bias")):
        _req(t, F32, n, 4)
    _req(out, F16, "out")
    B, Cc, h, ww = z.shape
    check(_lib.lib().gl_latent_affine_pack(z.data_ptr(), w.data_ptr(), bias.data_ptr(), pre, B, Cc, h * ww, Cpad,
                                           out.data_ptr(), _stream()), "gl_latent_affine_pack")
    return out


def set_option(key: int, value: int) -> None:
    """Tuning knob for A/B measurements (see gl_set_option in include/gligen_hip.h)."""
    check(_lib.lib().gl_set_option(key, value), "gl_set_option")


def gemm8_launch_count() -> int:
    """gl_gemm / gl_conv3x3 calls this process has served with the 8-wave kernel (gl_debug_read(9)); the tests of that kernel
    assert it moved, so a dispatcher that quietly stopped choosing it cannot pass them."""
    import ctypes
    n = ctypes.c_uint64(0)
    check(_lib.lib().gl_debug_read(9, ctypes.byref(n), 8), "gl_debug_read")
    return int(n.value)


def kxreuse_launch_count() -> int:
    """gl_conv3x3 calls this process has served with the kx-reuse loop of the 8-wave kernel (gl_debug_read(11), option key 54)."""
    import ctypes
    n = ctypes.c_uint64(0)
    check(_lib.lib().gl_debug_read(11, ctypes.byref(n), 8), "gl_debug_read")
    return int(n.value)


def upfold_launch_count() -> int:
    """gl_conv3x3 calls this process has served as folded upsample convs (gl_debug_read(12), gl_conv_args.upsample2x = 2)."""
    import ctypes
    n = ctypes.c_uint64(0)
    check(_lib.lib().gl_debug_read(12, ctypes.byref(n), 8), "gl_debug_read")
    return int(n.value)


ATTN_FORMS = ("split_pipe", "split_8w", "split_4w_dbuf", "split_4w_single", "f16_8w_pre0", "f16_8w_pre1", "f16_8w_pre2", "f16_4w_pre0",
              "f16_4w_pre1", "f16_4w_pre2")


def attention_launch_counts() -> dict:
    """gl_attention calls this process has served, per kernel form (gl_debug_read(10), names in ATTN_FORMS): the tests assert that the form
    they mean to test, and only that one, took their launches."""
    import ctypes
    n = (ctypes.c_uint64 * len(ATTN_FORMS))()
    check(_lib.lib().gl_debug_read(10, ctypes.byref(n), ctypes.sizeof(n)), "gl_debug_read")
    return {k: int(v) for k, v in zip(ATTN_FORMS, n)}


# ------------------------------------------------------------------------------------------- CLIP towers (reward stage)
def clip_patchify(pixel_values: torch.Tensor, patch: int, Kpad: int, out: torch.Tensor) -> torch.Tensor:
    """pixel_values fp32 [B, 3, S, S] -> fp16 [B * (S/patch)^2, Kpad] patch rows (K index (c, i, j), zero-padded)."""
    _req(pixel_values, F32, "pixel_values")
    _req(out, F16, "out")
    B, c3, S, S2 = pixel_values.shape
    if c3 != 3 or S != S2 or not pixel_values.is_contiguous():
        raise ValueError("pixel_values must be a contiguous [B, 3, S, S] tensor")
    check(_lib.lib().gl_clip_patchify(pixel_values.data_ptr(), B, S, patch, Kpad, out.data_ptr(), _stream()), "gl_clip_patchify")
    return out


def clip_assemble(patch_emb: torch.Tensor, class_emb: torch.Tensor, pos_emb: torch.Tensor, B: int, T: int, x: torch.Tensor,
                  ln_gamma: Optional[torch.Tensor] = None, ln_beta: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    _req(patch_emb, F16, "patch_emb")
    for t, n in ((class_emb, "class_emb"), (pos_emb, "pos_emb"), (x, "x")):
        _req(t, F32, n)
    C_ = x.shape[-1]
    check(_lib.lib().gl_clip_assemble(patch_emb.data_ptr(), _rows(patch_emb, "patch_emb")[2], class_emb.data_ptr(), pos_emb.data_ptr(), B, T, C_,
                                      _ptr(ln_gamma), _ptr(ln_beta), eps, x.data_ptr(), _stream()), "gl_clip_assemble")
    return x


def clip_embed_tokens(ids: torch.Tensor, tok_emb: torch.Tensor, pos_emb: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    _req(ids, torch.int32, "ids", 4)
    for t, n in ((tok_emb, "tok_emb"), (pos_emb, "pos_emb"), (x, "x")):
        _req(t, F32, n)
    B, T = ids.shape
    check(_lib.lib().gl_clip_embed_tokens(ids.data_ptr(), tok_emb.data_ptr(), pos_emb.data_ptr(), B, T, x.shape[-1], tok_emb.shape[0],
                                          x.data_ptr(), _stream()), "gl_clip_embed_tokens")
    return x


def clip_gather_rows(x: torch.Tensor, rows: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _req(x, F32, "x")
    _req(rows, torch.int32, "rows", 4)
    _req(out, F32, "out")
    check(_lib.lib().gl_clip_gather_rows(x.data_ptr(), _rows(x, "x")[2], rows.data_ptr(), rows.numel(), x.shape[-1], out.data_ptr(), _stream()),
          "gl_clip_gather_rows")
    return out


def attention_small(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, ld: int, B: int, T: int, H: int, d: int, scale: float,
                    causal: bool, out: torch.Tensor) -> torch.Tensor:
    """q / k / v: fp16 views whose element (b, t, h*d + c) sits at data_ptr + (b*T + t)*ld + h*d + c; out fp16 [B*T, H*d]."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _req(t, F16, n, 2)
    _req(out, F16, "out", 2)
    check(_lib.lib().gl_attention_small(q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, B, T, H, d, scale, int(causal), out.data_ptr(),
                                        _rows(out, "out")[2], _stream()), "gl_attention_small")
    return out


# ------------------------------------------------------------------------------------------- reward-stage image preprocessing
def image_to_u8(img: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """decoded image fp32 [B, 3, H, W] -> uint8 [B, H, W, 3] (interface.py:543-547 arithmetic)."""
    _req(img, F32, "img")
    B, c3, H, W = img.shape
    if c3 != 3 or not img.is_contiguous() or out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous():
        raise ValueError("img must be contiguous fp32 [B, 3, H, W] and out contiguous uint8 [B, H, W, 3]")
    check(_lib.lib().gl_image_to_u8(img.data_ptr(), B, H, W, out.data_ptr(), _stream()), "gl_image_to_u8")
    return out


def _req_tables(bounds: torch.Tensor, coeffs: torch.Tensor, n_out: int, ksize: int) -> None:
    if bounds.dtype != torch.int32 or coeffs.dtype != torch.int32 or not bounds.is_cuda or not coeffs.is_cuda:
        raise ValueError("bounds / coeffs must be int32 tensors on the GPU")
    if tuple(bounds.shape) != (n_out, 2) or tuple(coeffs.shape) != (n_out, ksize) or not bounds.is_contiguous() or not coeffs.is_contiguous():
        raise ValueError("bounds must be [n_out, 2] and coeffs [n_out, ksize], contiguous")


def resample_h_u8(x: torch.Tensor, bounds: torch.Tensor, coeffs: torch.Tensor, ksize: int, out: torch.Tensor) -> torch.Tensor:
    """Pillow's horizontal 8-bit resampling pass: uint8 [B, H, W, 3] -> uint8 [B, H, Wout, 3]."""
    if x.dtype != torch.uint8 or out.dtype != torch.uint8 or not x.is_cuda or not out.is_cuda or not x.is_contiguous() or not out.is_contiguous():
        raise ValueError("x / out must be contiguous uint8 tensors on the GPU")
    B, H, W, _ = x.shape
    Wout = out.shape[2]
    if tuple(out.shape) != (B, H, Wout, 3):
        raise ValueError("out must be [B, H, Wout, 3]")
    _req_tables(bounds, coeffs, Wout, ksize)
    check(_lib.lib().gl_resample_h_u8(x.data_ptr(), B, H, W, bounds.data_ptr(), coeffs.data_ptr(), ksize, Wout, out.data_ptr(), _stream()),
          "gl_resample_h_u8")
    return out


def resample_v_norm(x: torch.Tensor, bounds: torch.Tensor, coeffs: torch.Tensor, ksize: int, Hout: int, top: int, left: int, crop_h: int,
                    crop_w: int, mean, std, out: Optional[torch.Tensor], out_u8: Optional[torch.Tensor] = None):
    """Pillow's vertical pass inside the centre-crop window + /255, (x - mean) / std, channels first."""
    import ctypes

    import numpy as np
    if x.dtype != torch.uint8 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be a contiguous uint8 tensor on the GPU")
    B, H, W, _ = x.shape
    _req_tables(bounds, coeffs, Hout, ksize)
    if out is not None and (out.dtype != F32 or tuple(out.shape) != (B, 3, crop_h, crop_w) or not out.is_contiguous()):
        raise ValueError("out must be contiguous fp32 [B, 3, crop_h, crop_w]")
    if out_u8 is not None and (out_u8.dtype != torch.uint8 or tuple(out_u8.shape) != (B, crop_h, crop_w, 3) or not out_u8.is_contiguous()):
        raise ValueError("out_u8 must be contiguous uint8 [B, crop_h, crop_w, 3]")
    m = np.ascontiguousarray(mean, dtype=np.float32)
    s_ = np.ascontiguousarray(std, dtype=np.float32)
    check(_lib.lib().gl_resample_v_norm(x.data_ptr(), B, H, W, bounds.data_ptr(), coeffs.data_ptr(), ksize, Hout, top, left, crop_h, crop_w,
                                        m.ctypes.data_as(ctypes.c_void_p), s_.ctypes.data_as(ctypes.c_void_p),
                                        out.data_ptr() if out is not None else None, out_u8.data_ptr() if out_u8 is not None else None,
                                        _stream()), "gl_resample_v_norm")
    return out


# ---------------------------------------------------------------------------------------------------------------- spatial grounding (spatial.hip)
def _c32(t: torch.Tensor, name: str) -> None:
    _req(t, F32, name, 4)
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def sp_stem_patchify(map_: torch.Tensor, R: int, out: torch.Tensor) -> torch.Tensor:
    """map fp32 [B, 3, S, S] -> nearest resize to R x R -> fp16 patch rows [B * (R/4)^2, 64] of the 4x4 stride-4 stem conv (gl_sp_stem_patchify)"""
    _c32(map_, "map")
    if map_.dim() != 4 or map_.shape[1] != 3 or map_.shape[2] != map_.shape[3] or R % 4:
        raise ValueError(f"map {tuple(map_.shape)}: need [B, 3, S, S] and R % 4 == 0")
    B, S = map_.shape[0], map_.shape[2]
    _req(out, F16, "out")
    if not out.is_contiguous() or tuple(out.shape) != (B * (R // 4) ** 2, 64):
        raise ValueError(f"out: need a contiguous [{B * (R // 4) ** 2}, 64] tensor")
    check(_lib.lib().gl_sp_stem_patchify(map_.data_ptr(), B, S, R, out.data_ptr(), _stream()), "gl_sp_stem_patchify")
    return out


def sp_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """LayerNorm (eps 1e-6) over the columns of fp32 rows [M, C], fp32 out (``y`` may be ``x``)"""
    for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (y, "y")):
        _c32(t, n)
    M, C = x.shape
    if tuple(y.shape) != (M, C) or gamma.numel() != C or beta.numel() != C:
        raise ValueError("sp_layernorm: inconsistent shapes")
    check(_lib.lib().gl_sp_layernorm(x.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _stream()), "gl_sp_layernorm")
    return y


def sp_dwconv_ln(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, B: int, H: int, W: int,
                 out: torch.Tensor) -> torch.Tensor:
    """x fp32 NHWC rows [B * H * W, C], w fp32 [49, C] (tap-major depthwise 7x7), -> LayerNorm (eps 1e-6) -> fp16 [B * H * W, ldo], ldo = C rounded
    up to 64 with zero pad columns (gl_sp_dwconv_ln)"""
    for t, n in ((x, "x"), (w, "w"), (bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        _c32(t, n)
    C = x.shape[-1]
    if x.numel() != B * H * W * C or tuple(w.shape) != (49, C) or bias.numel() != C or gamma.numel() != C or beta.numel() != C:
        raise ValueError("sp_dwconv_ln: inconsistent shapes")
    _req(out, F16, "out")
    if out.dim() != 2 or not out.is_contiguous() or out.shape[0] != B * H * W or out.shape[1] % 64 or out.shape[1] < C:
        raise ValueError(f"out: need a contiguous [{B * H * W}, C rounded up to 64] tensor")
    check(_lib.lib().gl_sp_dwconv_ln(x.data_ptr(), w.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B, H, W, C, out.shape[1],
                                     out.data_ptr(), _stream()), "gl_sp_dwconv_ln")
    return out


def sp_gelu(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """erf-GELU on contiguous fp16 values (gl_sp_gelu); ``y`` may be ``x``"""
    _req(x, F16, "x", 4)
    _req(y, F16, "y", 4)
    if not x.is_contiguous() or not y.is_contiguous() or x.numel() != y.numel() or x.numel() % 2:
        raise ValueError("sp_gelu: contiguous tensors of one even size")
    check(_lib.lib().gl_sp_gelu(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "gl_sp_gelu")
    return y


def sp_down_gather(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, B: int, H: int, W: int, out: torch.Tensor) -> torch.Tensor:
    """x fp32 NHWC rows [B * H * W, C] -> per-pixel LayerNorm -> fp16 [B * H/2 * W/2, 4 C], the operand of the 2x2 stride-2 conv (gl_sp_down_gather)"""
    for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
        _c32(t, n)
    C = x.shape[-1]
    _req(out, F16, "out")
    if x.numel() != B * H * W * C or H % 2 or W % 2 or not out.is_contiguous() or tuple(out.shape) != (B * (H // 2) * (W // 2), 4 * C) or \
            gamma.numel() != C or beta.numel() != C:
        raise ValueError("sp_down_gather: inconsistent shapes")
    check(_lib.lib().gl_sp_down_gather(x.data_ptr(), B, H, W, C, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), _stream()), "gl_sp_down_gather")
    return out


def sp_assemble(feat: torch.Tensor, mask: torch.Tensor, null_feature: torch.Tensor, pos: torch.Tensor, B: int, T: int, out: torch.Tensor) -> torch.Tensor:
    """feat fp32 [B * T, C], mask [B], null_feature [C], pos [T, C] -> fp16 [B * T, C] = feat * m + null * (1 - m) + pos (gl_sp_assemble)"""
    for t, n in ((feat, "feat"), (mask, "mask"), (null_feature, "null_feature"), (pos, "pos")):
        _c32(t, n)
    C = feat.shape[-1]
    _req(out, F16, "out")
    if tuple(feat.shape) != (B * T, C) or mask.numel() != B or null_feature.numel() != C or pos.numel() != T * C or not out.is_contiguous() or \
            tuple(out.shape) != (B * T, C):
        raise ValueError("sp_assemble: inconsistent shapes")
    check(_lib.lib().gl_sp_assemble(feat.data_ptr(), mask.data_ptr(), null_feature.data_ptr(), pos.data_ptr(), B, T, C, out.data_ptr(), _stream()),
          "gl_sp_assemble")
    return out


def sp_bicubic(x: torch.Tensor, C: int, iy: torch.Tensor, wy: torch.Tensor, ix: torch.Tensor, wx: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Bicubic resize of the first C channels of x fp32 [B, Ct, Hin, Win] from index / weight tables [Hout | Wout, 4] (spatial.bicubic_table)"""
    _c32(x, "x")
    _c32(wy, "wy")
    _c32(wx, "wx")
    _c32(out, "out")
    _req(iy, torch.int32, "iy", 4)
    _req(ix, torch.int32, "ix", 4)
    B, Ct, Hin, Win = x.shape
    Hout, Wout = iy.shape[0], ix.shape[0]
    if tuple(iy.shape) != (Hout, 4) or tuple(wy.shape) != (Hout, 4) or tuple(ix.shape) != (Wout, 4) or tuple(wx.shape) != (Wout, 4) or \
            not iy.is_contiguous() or not ix.is_contiguous() or tuple(out.shape) != (B, C, Hout, Wout) or not 1 <= C <= Ct:
        raise ValueError("sp_bicubic: inconsistent shapes")
    if int(iy.min()) < 0 or int(iy.max()) >= Hin or int(ix.min()) < 0 or int(ix.max()) >= Win:
        raise ValueError("sp_bicubic: a table index lies outside the input")
    check(_lib.lib().gl_sp_bicubic(x.data_ptr(), B, Ct, C, Hin, Win, iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr(), Hout, Wout,
                                   out.data_ptr(), _stream()), "gl_sp_bicubic")
    return out


def sp_conv4x4s2(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, silu: bool, out: torch.Tensor) -> torch.Tensor:
    """Conv2d(Ci, Co, 4, 2, 1) on fp32 NCHW with an optional SiLU (gl_sp_conv4x4s2); Ci, Co <= 8"""
    for t, n in ((x, "x"), (w, "w"), (bias, "bias"), (out, "out")):
        _c32(t, n)
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    if tuple(w.shape) != (Co, Ci, 4, 4) or bias.numel() != Co or H % 2 or W % 2 or tuple(out.shape) != (B, Co, H // 2, W // 2):
        raise ValueError("sp_conv4x4s2: inconsistent shapes")
    check(_lib.lib().gl_sp_conv4x4s2(x.data_ptr(), w.data_ptr(), bias.data_ptr(), B, Ci, Co, H, W, int(bool(silu)), out.data_ptr(), _stream()),
          "gl_sp_conv4x4s2")
    return out


# ---------------------------------------------------------------------------------------------------------------- semantic-map grounding (sem.hip)
def sem_gather_conv(cmap: torch.Tensor, R: int, table: torch.Tensor, bias: torch.Tensor, K: int, stride: int, pad: int, silu: bool,
                    out: torch.Tensor) -> torch.Tensor:
    """class map uint8 [B, Hs, Ws] -> nearest resize to R x R -> Conv2d(classes, Co, K, stride, pad) of its one-hot as a gather from ``table``
    fp32 [classes, K * K, Co padded to 4] (semantic.gather_table) (+ SiLU) -> fp32 [B, Co, Ro, Ro] (gl_sem_gather_conv)"""
    _req(cmap, torch.uint8, "cmap", 1)
    _req(table, F32, "table", 16)
    _c32(bias, "bias")
    _c32(out, "out")
    Co = bias.numel()
    if cmap.dim() != 3 or not cmap.is_contiguous() or table.dim() != 3 or not table.is_contiguous() or table.shape[1] != K * K or \
            table.shape[2] != (Co + 3) // 4 * 4:
        raise ValueError(f"sem_gather_conv: need a contiguous uint8 [B, Hs, Ws] map and a contiguous table [classes, {K * K}, {(Co + 3) // 4 * 4}]")
    B, Hs, Ws = cmap.shape
    Ro = (R + 2 * pad - K) // stride + 1
    if tuple(out.shape) != (B, Co, Ro, Ro):
        raise ValueError(f"out: need [{B}, {Co}, {Ro}, {Ro}]")
    check(_lib.lib().gl_sem_gather_conv(cmap.data_ptr(), B, Hs, Ws, R, table.data_ptr(), bias.data_ptr(), table.shape[0], K, stride, pad, Co,
                                        int(bool(silu)), out.data_ptr(), _stream()), "gl_sem_gather_conv")
    return out


def sem_conv4x4s2(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Conv2d(Ci, Co, 4, 2, 1) on fp32 NCHW (gl_sem_conv4x4s2); Ci, Co <= 64"""
    for t, n in ((x, "x"), (w, "w"), (bias, "bias"), (out, "out")):
        _c32(t, n)
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    if tuple(w.shape) != (Co, Ci, 4, 4) or bias.numel() != Co or H % 2 or W % 2 or tuple(out.shape) != (B, Co, H // 2, W // 2):
        raise ValueError("sem_conv4x4s2: inconsistent shapes")
    check(_lib.lib().gl_sem_conv4x4s2(x.data_ptr(), w.data_ptr(), bias.data_ptr(), B, Ci, Co, H, W, out.data_ptr(), _stream()), "gl_sem_conv4x4s2")
    return out


def sem_onehot_index(x: torch.Tensor, out: torch.Tensor, bad: torch.Tensor) -> torch.Tensor:
    """fp32 one-hot [B, C, H, W] -> uint8 class map [B, H, W] (argmax) and ``bad`` int32 [B], the pixels of each sample that are not exactly
    one-hot (gl_sem_onehot_index)"""
    _c32(x, "x")
    _req(out, torch.uint8, "out", 1)
    _req(bad, torch.int32, "bad", 4)
    if x.dim() != 4 or not out.is_contiguous() or tuple(out.shape) != (x.shape[0], x.shape[2], x.shape[3]) or not bad.is_contiguous() or \
            bad.numel() != x.shape[0]:
        raise ValueError("sem_onehot_index: need x [B, C, H, W], out uint8 [B, H, W] and bad int32 [B]")
    B, C, H, W = x.shape
    check(_lib.lib().gl_sem_onehot_index(x.data_ptr(), B, C, H, W, out.data_ptr(), bad.data_ptr(), _stream()), "gl_sem_onehot_index")
    return out
