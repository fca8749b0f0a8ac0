"""Checkpoint ingestion: reference-named fp32 state_dict -> packed fp16/fp32 device tensors.

The engine never sees torch modules; it consumes the flat dict this module produces.  Packing is
layout work only (no arithmetic beyond dtype casts and tanh of the scalar gates):

  * Linear / 1x1-conv weights  [N, K]            -> fp16 [N, K]
  * 3x3 conv weights [Cout, Cin, 3, 3]          -> fp16 [Cout, 9*Cin], K = (64-channel block, tap, channel) (NHWC implicit GEMM);
                                                   the 4-channel first conv is zero-padded to Cin = 64
  * Upsample conv weights [Cout, Cin, 3, 3]     -> fp16 [4*Cout, 4*Cin]: one 2x2 kernel per output parity, summed in fp32 (pack_conv_upfold;
                                                   option key 55, not in a split_weights table)
  * GEGLU proj [8C, C] (x rows | gate rows)      -> rows interleaved in blocks of 32 (x32 | gate32 | x32 | ...)
                                                   so x_j and gate_j land in adjacent MFMA tiles (bias likewise)
  * self-attention to_q/to_k/to_v                -> one [3C, C] matrix (single QKV GEMM)
  * cross-attention to_k/to_v (context/relations)-> one [2C, 768] matrix (hoisted K/V GEMM)
  * the 22 ResBlock emb_layers                   -> one [sum Cout, 4*mc] matrix (one GEMM per step)
  * biases, norm affine params                   -> fp32
  * alpha_attn / alpha_dense                     -> tanh() as python floats (fuser: multiplied by the
                                                   sampler's scale per step; rela_fuse: constant)
State-dict names follow SURVEY.md App-C, so a real GLIGEN checkpoint's ``saved_ckpt['model']`` loads
(strict=False semantics, interface.py:91: missing keys raise here, unexpected keys are ignored).
"""
from __future__ import annotations

import math
from typing import Dict, Mapping

import numpy as np
import torch

from .arch import Plan, UNetConfig, build_plan, param_shapes

CIN_PAD = 64
LOG2E = 1.4426950408889634


def q_fold(d_head: int) -> float:
    """The softmax scale d^-1/2 (attention.py:136,172) times log2(e), folded into every q projection at pack time: the
    attention kernel then gets logits in exp2 units straight out of the MFMA (gl_attn_args.q_prescaled)."""
    return float(d_head) ** -0.5 * LOG2E


def pad64(k: int) -> int:
    """k rounded up to the GEMMs' K multiple (the row width of a keypoint model's position_net.linears.0 and of the rows it multiplies)"""
    return (k + 63) // 64 * 64


def _t(v, device) -> torch.Tensor:
    if not torch.is_tensor(v):
        v = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
    return v.to(device=device, dtype=torch.float32)


def _h(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float16).contiguous()


def pack_conv3x3(w: torch.Tensor, cin_pad: int | None = None) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> fp16 [Cout, 9*Cin] with K ordered (64-channel block, tap, channel-in-block): the
    implicit-GEMM kernel then visits the 9 taps of one channel block back to back (cache-hot halo reuse)."""
    cout, cin = w.shape[0], w.shape[1]
    if cin_pad is not None and cin_pad > cin:
        z = torch.zeros(cout, cin_pad - cin, 3, 3, dtype=w.dtype, device=w.device)
        w = torch.cat([w, z], dim=1)
        cin = cin_pad
    assert cin % 64 == 0, "conv input channels must be a multiple of 64 (pad the first conv)"
    wp = w.reshape(cout, cin // 64, 64, 3, 3).permute(0, 1, 3, 4, 2)    # [Cout, Cin/64, 3, 3, 64]
    return _h(wp.reshape(cout, -1))


# taps of the 3x3 kernel that window position a (or b) of output parity py (or px) collects: S[parity][position]
UPFOLD_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))


# Narrowest upsample conv (channels) of a UNet config whose up convs are folded under the default of option key 55 (2): the full model's 640- and
# 1280-channel layers run in 0.42-0.54 of the 9-tap time at 2B = 8 (-0.31 ms per forward).  Narrower configs exist only at test size: there the
# folded launch is faster too, but by 3-7 us of a latency-bound launch (profiles/upfold_shapes.txt), and their compact pack stays what it was --
# bit-identical to the Whi half of the split_weights pack of the same checkpoint, which never folds.  fold_up=True or key 55 = 1 folds any config.
# Static per config: never a function of batch or map size.
UPFOLD_MIN_CHANNELS = 512


def fold_up_rule(cfg: UNetConfig) -> bool:
    ups = [l.cin for l in build_plan(cfg).all_layers() if l.kind == "up"]
    return bool(ups) and min(ups) >= UPFOLD_MIN_CHANNELS and not cfg.split_weights


def pack_conv_upfold(w32: torch.Tensor) -> torch.Tensor:
    """Upsample conv [Cout, Cin, 3, 3] fp32 -> fp16 [4*Cout, 4*Cin].  After nearest-2x upsampling the nine taps of output pixel
    (2y + py, 2x + px) touch only the source pixels (y + py - 1 + a, x + px - 1 + b), a, b in {0, 1}: per parity the layer is a 2x2 conv on the
    source grid with Wf[py,px][:, :, a, b] = sum of W[:, :, ky, kx] over ky in S(py, a), kx in S(px, b).  The sums are taken in fp32 from the
    unrounded weights and rounded ONCE.  Rows (parity py * 2 + px, Cout); K ordered (64-channel block, tap a * 2 + b, channel in block)."""
    w32 = w32.float()
    cout, cin = w32.shape[0], w32.shape[1]
    assert tuple(w32.shape[2:]) == (3, 3) and cin % 64 == 0, "upsample conv: 3x3 kernel, input channels a multiple of 64"
    out = []
    for py in range(2):
        for px in range(2):
            f = torch.zeros(cout, cin, 2, 2, dtype=torch.float32, device=w32.device)
            for a in range(2):
                for b in range(2):
                    for ky in UPFOLD_TAPS[py][a]:
                        for kx in UPFOLD_TAPS[px][b]:
                            f[:, :, a, b] += w32[:, :, ky, kx]
            out.append(f.reshape(cout, cin // 64, 64, 2, 2).permute(0, 1, 3, 4, 2).reshape(cout, -1))
    return _h(torch.cat(out, 0))


def pack_first_conv(w: torch.Tensor, cin_pad: int) -> torch.Tensor:
    """first conv [Cout, C, 3, 3] fp32 (C = 4 latent channels of 64 padded ones; C = 9 on an inpaint_mode model: 27 of 64): input channels
    [Whi | Whi | Wlo | 0] for the latent packed as [hi | lo | hi] (gl_pack_latent / gl_pack_latent_extra split): x.W = xhi.Whi + xlo.Whi + xhi.Wlo at no cost.  The first conv alone carries 7 % of the error of storing
    the UNet's weights in fp16 (profiles/r4_weight_rounding_attribution.txt)."""
    w = w.float()
    if 3 * w.shape[1] > cin_pad:
        return pack_conv3x3(w, cin_pad)
    hi = w.half().float()
    lo = (w - hi).half().float()
    return pack_conv3x3(torch.cat([hi, hi, lo], dim=1), cin_pad)


def geglu_interleave(t: torch.Tensor) -> torch.Tensor:
    """rows [x (4C) | gate (4C)] -> blocks of 32: x[0:32], gate[0:32], x[32:64], gate[32:64], ..."""
    half = t.shape[0] // 2
    assert half % 32 == 0, "GEGLU inner dim must be a multiple of 32"
    x = t[:half].reshape(half // 32, 1, 32, *t.shape[1:])
    g = t[half:].reshape(half // 32, 1, 32, *t.shape[1:])
    return torch.cat([x, g], dim=1).reshape(t.shape)


def flat_views(table, total, device, flat=None):
    """An engine handle's weight table (_lib.weight_table / vae_weight_table) -> the flat byte buffer of ``total`` bytes (zeros, unless an
    already filled ``flat`` is given) and its {name: typed view}, in table order."""
    if flat is None:
        flat = torch.zeros(total, dtype=torch.uint8, device=device)
    return flat, {name: flat[off:off + nbytes].view(torch.float16 if dtype == 0 else torch.float32).view(shape)
                  for name, off, nbytes, dtype, shape in table}


def copy_packed(name: str, dst: torch.Tensor, src: torch.Tensor) -> None:
    """One packed tensor into its view of the flat buffer: the packer and the engine table must agree on shape and dtype."""
    if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        raise ValueError(f"{name}: packed {tuple(src.shape)} {src.dtype} != engine table {tuple(dst.shape)} {dst.dtype}")
    dst.copy_(src)


class PackedWeights:
    """``w[name]`` packed tensors + python scalars ``s[name]``.  After ``to_flat()`` every tensor is a VIEW into one
    flat byte buffer ``flat`` whose layout is defined by the C engine's weight table (gl_weight_at, include/gligen_hip.h):
    that buffer is what gl_load_weights consumes and what dist.broadcast_packed sends in one collective."""

    def __init__(self, cfg: UNetConfig, plan: Plan, device):
        self.cfg, self.plan, self.device = cfg, plan, device
        self.w: Dict[str, torch.Tensor] = {}
        self.s: Dict[str, float] = {}
        self.emb_offsets: Dict[str, int] = {}
        self.emb_total = 0
        self.flat: torch.Tensor | None = None
        self.has_sd_conv = False
        self.fold_up: bool | None = None         # upsample convs packed as folded 2x2 kernels (None: the handle default, 9-tap rows unless key 55 = 1)

    def nbytes(self) -> int:
        return int(self.flat.numel()) if self.flat is not None else sum(t.numel() * t.element_size() for t in self.w.values())

    def to_flat(self) -> "PackedWeights":
        """Moves every packed tensor into the flat buffer at the offsets the C engine dictates and rebinds ``w`` to views."""
        from . import _lib
        flat, views = flat_views(*_lib.engine_table(self.cfg, self.fold_up), self.device)
        self.has_sd_conv = "sd_first_conv.w" in self.w
        for name, dst in views.items():
            if name in self.w:
                copy_packed(name, dst, self.w[name])
            elif name in self.s:
                dst.fill_(float(self.s[name]))
                self.s[name] = float(dst.item())       # the gates are fp32 on the device: keep the host copy identical
            elif name.startswith("sd_first_conv."):
                pass                                   # no SD conv given: slot stays zero, gl_load_weights(has_sd_conv=0)
            else:
                raise KeyError(f"engine weight table wants {name}, which the packer did not produce")
        extra = set(self.w) - set(views)
        if extra:
            raise KeyError(f"packer produced tensors the engine does not know: {sorted(extra)[:3]}")
        self.w, self.flat = views, flat
        return self

    @staticmethod
    def from_flat(flat: torch.Tensor, cfg: UNetConfig, device, has_sd_conv: bool, fold_up: bool | None = None) -> "PackedWeights":
        """Rebuilds the views (and the scalar gates) from a flat buffer, e.g. on the receiving ranks of the broadcast.
        ``fold_up``: whether the buffer was packed with folded upsample convs (None: what pack_state_dict would do now)."""
        from . import _lib
        P = PackedWeights(cfg, build_plan(cfg), device)
        P.fold_up = fold_up = _lib.resolve_fold_up(fold_up, fold_up_rule(cfg))
        table, total = _lib.engine_table(cfg, fold_up)
        if flat.numel() != total:
            raise ValueError(f"flat buffer has {flat.numel()} bytes, the engine table needs {total}")
        _, P.w = flat_views(table, total, device, flat)
        P.s = {name: float(v.item()) for name, v in P.w.items() if name.endswith((".tanh_attn", ".tanh_dense"))}
        off = 0
        for l in P.plan.all_layers():
            if l.kind == "res":
                P.emb_offsets[l.prefix] = off
                off += l.cout
        P.emb_total = off
        P.flat, P.has_sd_conv = flat, has_sd_conv
        return P


def pack_state_dict(sd: Mapping[str, object], cfg: UNetConfig, device, sd_first_conv: Mapping[str, object] | None = None,
                    fold_up: bool | None = None) -> PackedWeights:
    """``fold_up``: upsample convs as folded 2x2 kernels (pack_conv_upfold); None = the current value of option key 55, whose default
    folds the configs of ``fold_up_rule``.  A split_weights pack never folds."""
    plan = build_plan(cfg)
    need = param_shapes(cfg)
    missing = [k for k in need if k not in sd]
    if missing:
        raise KeyError(f"state_dict is missing {len(missing)} tensors, e.g. {missing[:3]}")
    for k, shp in need.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != expected {shp}")
    if sd_first_conv is not None and cfg.inpaint_mode:
        # openaimodel.py:296: first_conv_restorable = False -- the 4-channel SD conv cannot take the 9-channel input
        raise ValueError("an inpaint_mode model has no SD first conv (its first conv is not restorable, openaimodel.py:296)")
    P = PackedWeights(cfg, plan, device)
    W, S = P.w, P.s
    g = lambda k: _t(sd[k], device)
    split_all = bool(cfg.split_weights)
    from . import _lib
    P.fold_up = _lib.resolve_fold_up(fold_up, fold_up_rule(cfg))
    fold = P.fold_up and not split_all

    def mat(w32: torch.Tensor) -> torch.Tensor:
        """fp32 [N, K] -> the stored matrix: fp16 [N, K], or rows [Whi | Wlo] (fp16 [N, 2K]) in a split_weights table
        (gl_unet_config.split_weights: strict mode's third pass x.Wlo restores the fp32 weight to ~22 bits)"""
        w32 = w32.reshape(w32.shape[0], -1).float()
        hi = _h(w32)
        if not split_all:
            return hi
        return torch.cat([hi, _h(w32 - hi.float())], 1).contiguous()

    def lin(p, dst=None, bias=True):
        dst = dst or p
        W[dst + ".w"] = mat(g(p + ".weight"))
        if bias:
            W[dst + ".b"] = g(p + ".bias").contiguous()

    def lin_split(p):
        """the three kinds of 1x1 conv: rows [Whi | Wlo], Whi = fp16(W), Wlo = fp16(W - Whi) (engine.hip add_lin_split; they carry 57 % of the
        error of storing the weights in fp16, profiles/r4_weight_rounding_attribution.txt)"""
        w32 = g(p + ".weight").reshape(g(p + ".weight").shape[0], -1).float()
        hi = _h(w32)
        lo = _h(w32 - hi.float())
        W[p + ".w"] = torch.cat([hi, lo], 1).contiguous()
        W[p + ".b"] = g(p + ".bias").contiguous()

    def norm(p):
        W[p + ".g"] = g(p + ".weight").contiguous()
        W[p + ".b"] = g(p + ".bias").contiguous()

    def conv3(p, cin_pad=None):
        w32 = g(p + ".weight").float()
        hi = pack_conv3x3(w32, cin_pad)
        if split_all:        # rows [Whi | Wlo], each half in the (64-channel block, tap, channel) order (gl_conv_args.w_split)
            lo = pack_conv3x3(w32 - w32.half().float(), cin_pad)
            hi = torch.cat([hi, lo], 1).contiguous()
        W[p + ".w"] = hi
        W[p + ".b"] = g(p + ".bias").contiguous()

    def ff(p):
        W[p + ".ff1.w"] = mat(geglu_interleave(g(p + ".net.0.proj.weight")))
        W[p + ".ff1.b"] = geglu_interleave(g(p + ".net.0.proj.bias")).contiguous()
        lin(p + ".net.2", p + ".ff2")

    def self_attn(p, d):
        W[p + ".qkv.w"] = mat(torch.cat([g(p + ".to_q.weight") * q_fold(d), g(p + ".to_k.weight"), g(p + ".to_v.weight")], 0))
        lin(p + ".to_out.0", p + ".o")

    def cross_attn(p, d):
        W[p + ".q.w"] = mat(g(p + ".to_q.weight") * q_fold(d))
        W[p + ".kv.w"] = mat(torch.cat([g(p + ".to_k.weight"), g(p + ".to_v.weight")], 0))
        lin(p + ".to_out.0", p + ".o")

    lin("time_embed.0")
    lin("time_embed.2")
    # first conv: GLIGEN's own and the "SD" replacement (openaimodel.py:393-405)
    W["input_blocks.0.0.w"] = pack_first_conv(g("input_blocks.0.0.weight"), CIN_PAD)
    W["input_blocks.0.0.b"] = g("input_blocks.0.0.bias").contiguous()
    if sd_first_conv is not None:
        W["sd_first_conv.w"] = pack_first_conv(_t(sd_first_conv["weight"], device), CIN_PAD)
        W["sd_first_conv.b"] = _t(sd_first_conv["bias"], device).contiguous()

    emb_w, emb_b, off = [], [], 0
    for l in plan.all_layers():
        p = l.prefix
        if l.kind == "up" and fold:
            W[p + ".w"] = pack_conv_upfold(g(p + ".weight"))
            W[p + ".b"] = g(p + ".bias").contiguous()
        elif l.kind in ("down", "up"):
            conv3(p)
        elif l.kind == "res":
            norm(p + ".in_layers.0")
            conv3(p + ".in_layers.2")
            norm(p + ".out_layers.0")
            conv3(p + ".out_layers.3")
            if l.cin != l.cout:
                lin_split(p + ".skip_connection")
            emb_w.append(g(p + ".emb_layers.1.weight"))
            emb_b.append(g(p + ".emb_layers.1.bias"))
            P.emb_offsets[p] = off
            off += l.cout
        elif l.kind == "st":
            norm(p + ".norm")
            lin_split(p + ".proj_in")
            lin_split(p + ".proj_out")
            t = p + ".transformer_blocks.0"
            self_attn(t + ".attn1", l.d_head)
            cross_attn(t + ".attn2", l.d_head)
            ff(t + ".ff")
            for n in ("norm1", "norm2", "norm3"):
                norm(f"{t}.{n}")
            f = t + ".fuser"
            lin(f + ".linear")
            self_attn(f + ".attn", l.d_head)
            ff(f + ".ff")
            norm(f + ".norm1")
            norm(f + ".norm2")
            S[f + ".tanh_attn"] = math.tanh(float(g(f + ".alpha_attn")))
            S[f + ".tanh_dense"] = math.tanh(float(g(f + ".alpha_dense")))
            if not cfg.relation:
                continue                                # the upstream block (attention_original.py:312-316): no rela_fuse entries in the table either
            r = t + ".rela_fuse"
            cross_attn(r + ".attn", l.d_head)
            ff(r + ".ff")
            for n in ("norm1", "norm2", "norm3"):
                norm(f"{r}.{n}")
            S[r + ".tanh_attn"] = math.tanh(float(g(r + ".alpha_attn")))
            S[r + ".tanh_dense"] = math.tanh(float(g(r + ".alpha_dense")))
    W["emb_all.w"] = mat(torch.cat(emb_w, 0))
    W["emb_all.b"] = torch.cat(emb_b, 0).contiguous()
    P.emb_total = off
    norm("out.0")
    conv3("out.2")
    if cfg.grounding == "spatial":
        # the ConvNeXt tokenizer and the grounding downsampler are stages of their own (spatial.SpatialTokenizer / SpatialDownsampler pack
        # position_net.* and downsample_net.*): the handle takes finished tokens, its table has no position_net.* entries
        return P.to_flat()
    if cfg.grounding == "text_image":
        W["position_net.null_text"] = g("position_net.null_text_feature").contiguous()
        W["position_net.null_image"] = g("position_net.null_image_feature").contiguous()
        W["position_net.null_xyxy"] = g("position_net.null_position_feature").contiguous()
        for chain in ("linears_text", "linears_image"):
            for i in (0, 2, 4):
                lin(f"position_net.{chain}.{i}")
        return P.to_flat()
    if cfg.grounding == "keypoint":
        # the two tables and the two null features stay fp32 (the input kernel sums and blends them in fp32); linears.0 with its K = D + 4 F
        # columns zero-padded to the GEMMs' multiple of 64 (800 -> 832), each of the [Whi | Wlo] halves on its own in a split_weights table
        W["position_net.person_emb"] = g("position_net.person_embeddings").contiguous()
        W["position_net.keypoint_emb"] = g("position_net.keypoint_embeddings").contiguous()
        W["position_net.null_person"] = g("position_net.null_person_feature").contiguous()
        W["position_net.null_xy"] = g("position_net.null_xy_feature").contiguous()
        w0 = g("position_net.linears.0.weight")
        W["position_net.linears.0.w"] = mat(torch.nn.functional.pad(w0, (0, pad64(w0.shape[1]) - w0.shape[1])))
        W["position_net.linears.0.b"] = g("position_net.linears.0.bias").contiguous()
        for i in (2, 4):
            lin(f"position_net.linears.{i}")
        return P.to_flat()
    W["position_net.null_pos"] = g("position_net.null_positive_feature").contiguous()
    W["position_net.null_xyxy"] = g("position_net.null_position_feature").contiguous()
    for i in (0, 2, 4):
        lin(f"position_net.linears.{i}")
    return P.to_flat()


@torch.no_grad()
def random_state_dict(cfg: UNetConfig, device, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Fast on-device random weights with the recipe's *scaling rules* (not its values): used by the
    benchmark, where only shapes and magnitudes matter (no checkpoint is obtainable offline)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for name, shape in param_shapes(cfg).items():
        leaf = name.rsplit(".", 1)[-1]
        u = lambda: torch.rand(shape if len(shape) else (1,), generator=gen, device=device, dtype=torch.float32) * 2 - 1
        if leaf in ("alpha_attn", "alpha_dense"):
            v = u().reshape(())
            t = torch.sign(v) * (0.3 + 0.35 * v.abs())
        elif leaf.startswith("null_") or leaf in ("person_embeddings", "keypoint_embeddings", "pos_embedding"):
            t = u() * 0.5
        elif (".norm" in name or "in_layers.0" in name or "out_layers.0" in name or name.startswith("out.0")) and len(shape) == 1:
            t = 1.0 + 0.1 * u() if leaf == "weight" else 0.05 * u()
        elif leaf == "bias":
            t = 0.02 * u()
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            t = u() * math.sqrt(3.0 / max(fan_in, 1))
        out[name] = t
    return out


@torch.no_grad()
def random_vae_state_dict(cfg, device, seed: int = 1) -> Dict[str, torch.Tensor]:
    """On-device random VAE-decoder weights with the recipe's scaling rules (benchmark only)."""
    from .arch import vae_decoder_param_shapes
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for name, shape in vae_decoder_param_shapes(cfg).items():
        u = torch.rand(shape, generator=gen, device=device, dtype=torch.float32) * 2 - 1
        leaf = name.rsplit(".", 1)[-1]
        if "norm" in name and len(shape) == 1:
            out[name] = 1.0 + 0.1 * u if leaf == "weight" else 0.05 * u
        elif leaf == "bias":
            out[name] = 0.02 * u
        else:
            fan_in = 1
            for s_ in shape[1:]:
                fan_in *= s_
            out[name] = u * math.sqrt(3.0 / max(fan_in, 1))
    return out
