"""The two stages that the spatial grounding families (GLIGEN's canny / hed / depth / normal checkpoints) add in front of the UNet, on the
MI355X kernels; both run once per image, never per denoising step.

``SpatialTokenizer`` is ``{canny,hed,depth,normal}_grounding_net.PositionNet``: the map [B, 3, S, S] in [-1, 1] is resized (nearest) to
``resize_input``, run through a ConvNeXt (convnext.py: 4x4 stride-4 stem + LayerNorm, four stages of depthwise-7x7 / LayerNorm / Linear C -> 4C
/ erf-GELU / Linear 4C -> C / gamma / residual blocks with LayerNorm + 2x2 stride-2 convs between them, no final norm, no head), the
[B, 768, R/32, R/32] features become (R/32)^2 tokens, ``objs * mask + null_feature * (1 - mask) + pos_embedding``, then the three ``linears``.
Op-level orchestration like clip.py: every matrix product is ``ops.gemm`` (fp16 operands, fp32 accumulate) and the residual stream is fp32 NHWC
rows [B * H * W, C]; the stages in between are the kernels of csrc/spatial.hip.  ``gamma`` is folded into ``pwconv2`` at pack time
(``fold_gamma``), so the second pointwise GEMM adds straight onto the stream (EPI_RES); the erf-GELU is a kernel of its own between the two.

``SpatialDownsampler`` is ``*_grounding_downsampler.GroundingDownsampler``: channel 0 (normal: all 3) of ``grounding_extra_input``, torch's
bicubic resize, and for canny / depth / normal two 4x4 stride-2 convs with a SiLU between them; fp32 throughout.  Its output
[B, ds_out, h, w] is what ``UNetEngine.set_grounding_extra`` takes.

Nothing here fetches weights: the ConvNeXt comes from the checkpoint's own ``position_net.convnext_tiny_backbone.*`` tensors.  No fallback: a
missing GPU / library raises.
"""
from __future__ import annotations

from typing import Dict, Mapping, Tuple

import numpy as np
import torch

from .arch import HED_DS_SIZE, UNetConfig, spatial_tokenizer_params

F16, F32 = torch.float16, torch.float32
CUBIC_A = -0.75       # torch's bicubic coefficient (UpSample.h)


def pad64(k: int) -> int:
    return (k + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ index / weight tables (host, no device)
def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """Source index of every destination index of ``F.interpolate(mode="nearest")``: min(floor(dst * scale), n_in - 1), scale = n_in / n_out
    in fp32 as torch computes it (the stem kernel evaluates the same expression)."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1).astype(np.int32)


def bicubic_table(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """(index int32 [n_out, 4], weight fp32 [n_out, 4]) of ``F.interpolate(mode="bicubic", align_corners=False)`` along one axis, without
    antialias: source coordinate scale * (dst + 0.5) - 0.5 (NOT clamped at 0 for the cubic kernel), taps floor - 1 .. floor + 2 clamped to
    the input, coefficients of the A = -0.75 convolution kernel; fp32 arithmetic in torch's order of operations."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    real = scale * (np.arange(n_out, dtype=f) + f(0.5)) - f(0.5)
    fl = np.floor(real)
    t = (real - fl).astype(f)
    A = f(CUBIC_A)

    def cc1(x):       # |x| <= 1
        return ((A + f(2)) * x - (A + f(3))) * x * x + f(1)

    def cc2(x):       # 1 < |x| < 2
        return ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A
    w = np.stack([cc2(t + f(1)), cc1(t), cc1(f(1) - t), cc2(f(2) - t)], axis=1).astype(f)
    idx = fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    return np.clip(idx, 0, n_in - 1).astype(np.int32), w


# ------------------------------------------------------------------------------------------------ packing (any device, fp32 in)
def fold_gamma(gamma: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """convnext.py:44-46: ``gamma * (x W^T + b)`` as one Linear, (gamma (.) W, gamma (.) b) with gamma scaling the OUTPUT rows of W [C, 4C]"""
    return (gamma[:, None] * w).contiguous(), (gamma * b).contiguous()


def pack_tokenizer(sd: Mapping[str, object], cfg: UNetConfig, device) -> Dict[str, object]:
    """The tokenizer's tensors in the layouts its kernels read.  fp16 matrices [N, K] with K zero-padded to a multiple of 64 where the operand
    rows are (stem 48 -> 64, C = 96 -> 128); fp32 everything else.  A tensor the checkpoint lacks raises KeyError naming it."""
    need = spatial_tokenizer_params(cfg)
    for k, shp in need.items():
        if k not in sd:
            raise KeyError(f"spatial checkpoint is missing {k}")
        if tuple(sd[k].shape) != tuple(shp):
            raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != expected {shp}")
    g = lambda k: torch.as_tensor(np.asarray(sd[k]) if not torch.is_tensor(sd[k]) else sd[k]).detach().to(device, F32).contiguous()
    h = lambda t: t.to(F16).contiguous()
    padk = lambda w: torch.nn.functional.pad(w, (0, pad64(w.shape[1]) - w.shape[1]))
    dims, depths = cfg.convnext_dims, cfg.convnext_depths
    bb = "position_net.convnext_tiny_backbone"
    P: Dict[str, object] = {}
    P["stem.w"] = h(padk(g(bb + ".downsample_layers.0.0.weight").reshape(dims[0], 48)))        # K = (c * 4 + i) * 4 + j
    P["stem.b"] = g(bb + ".downsample_layers.0.0.bias")
    P["stem.ln"] = (g(bb + ".downsample_layers.0.1.weight"), g(bb + ".downsample_layers.0.1.bias"))
    for i in range(1, 4):
        P[f"down.{i}.ln"] = (g(bb + f".downsample_layers.{i}.0.weight"), g(bb + f".downsample_layers.{i}.0.bias"))
        w = g(bb + f".downsample_layers.{i}.1.weight")                                         # [Cout, Cin, 2, 2] -> [Cout, (ky, kx, Cin)]
        P[f"down.{i}.w"] = h(w.permute(0, 2, 3, 1).reshape(dims[i], 4 * dims[i - 1]))
        P[f"down.{i}.b"] = g(bb + f".downsample_layers.{i}.1.bias")
    blocks = []
    for i in range(4):
        C = dims[i]
        stage = []
        for j in range(depths[i]):
            p = bb + f".stages.{i}.{j}"
            w2, b2 = fold_gamma(g(p + ".gamma"), g(p + ".pwconv2.weight"), g(p + ".pwconv2.bias"))
            stage.append(dict(dw=g(p + ".dwconv.weight").reshape(C, 49).t().contiguous(), dwb=g(p + ".dwconv.bias"),        # tap-major [49, C]
                              ln=(g(p + ".norm.weight"), g(p + ".norm.bias")),
                              w1=h(padk(g(p + ".pwconv1.weight"))), b1=g(p + ".pwconv1.bias"), w2=h(w2), b2=b2))
        blocks.append(stage)
    P["stages"] = blocks
    P["pos"] = g("position_net.pos_embedding").reshape(cfg.n_ground, dims[3]).contiguous()
    P["null"] = g("position_net.null_feature")
    for i in (0, 2, 4):
        P[f"lin.{i}.w"] = h(g(f"position_net.linears.{i}.weight"))
        P[f"lin.{i}.b"] = g(f"position_net.linears.{i}.bias")
    return P


def backbone_of(sd: Mapping[str, object]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(depths, dims) of the ConvNeXt a checkpoint carries, read off its own ``position_net.convnext_tiny_backbone.*`` tensors (the config of a
    GLIGEN checkpoint does not state them: the reference hard-codes convnext_tiny)"""
    bb = "position_net.convnext_tiny_backbone"
    dims, depths = [], []
    for i in range(4):
        k = bb + f".downsample_layers.{i}.{0 if i == 0 else 1}.weight"
        if k not in sd:
            raise KeyError(f"spatial checkpoint is missing {k}")
        dims.append(int(sd[k].shape[0]))
        n = 0
        while bb + f".stages.{i}.{n}.dwconv.weight" in sd:
            n += 1
        depths.append(n)
    return tuple(depths), tuple(dims)


def check_tokenizer_cfg(cfg: UNetConfig) -> None:
    dims, R = cfg.convnext_dims, cfg.sp_resize_input
    if cfg.grounding != "spatial":
        raise ValueError(f"grounding = {cfg.grounding!r}: the ConvNeXt tokenizer belongs to the spatial families")
    if len(dims) != 4 or len(cfg.convnext_depths) != 4 or any(d % 16 or d > 768 for d in dims) or dims[3] % 64:
        raise NotImplementedError(f"ConvNeXt dims {dims}: four widths, multiples of 16 up to 768 (the last a multiple of 64)")
    if R % 32 or not 32 <= R <= 256:
        raise NotImplementedError(f"resize_input = {R}: a multiple of 32 up to 256 (64 grounding tokens at most)")
    if cfg.pos_out_dim % 8:
        raise NotImplementedError("out_dim must be a multiple of 8")


class SpatialTokenizer:
    def __init__(self, state_dict: Mapping[str, object], cfg: UNetConfig, device="cuda:0"):
        """``state_dict``: the checkpoint's ``model`` dict (``position_net.*`` names)."""
        if not torch.cuda.is_available():
            raise RuntimeError("SpatialTokenizer needs a GPU: the tokenizer stage has no CPU fallback")
        check_tokenizer_cfg(cfg)
        from ._lib import init_device
        init_device()
        self.cfg, self.device = cfg, torch.device(device)
        self.P = pack_tokenizer(state_dict, cfg, self.device)
        self.T, self.D = cfg.n_ground, cfg.pos_out_dim
        self._null = None

    def _linears(self, a: torch.Tensor) -> torch.Tensor:
        from . import ops
        from ._lib import EPI_BIAS, EPI_SILU
        P, M = self.P, a.shape[0]
        h1 = ops.gemm(a, P["lin.0.w"], torch.empty(M, 512, dtype=F16, device=self.device), P["lin.0.b"], EPI_SILU)
        h2 = ops.gemm(h1, P["lin.2.w"], torch.empty(M, 512, dtype=F16, device=self.device), P["lin.2.b"], EPI_SILU)
        return ops.gemm(h2, P["lin.4.w"], torch.empty(M, self.D, dtype=F32, device=self.device), P["lin.4.b"], EPI_BIAS)

    @torch.no_grad()
    def features(self, map_: torch.Tensor) -> torch.Tensor:
        """The ConvNeXt alone: map fp32 [B, 3, S, S] -> fp32 rows [B * T, dims[3]], row b * T + y * (R/32) + x"""
        from . import ops
        from ._lib import EPI_BIAS, EPI_RES
        cfg, P, dev = self.cfg, self.P, self.device
        px = torch.as_tensor(map_).to(dev, F32).contiguous()
        if px.dim() != 4 or px.shape[1] != 3 or px.shape[2] != px.shape[3]:
            raise ValueError(f"map {tuple(px.shape)}: need [B, 3, S, S]")
        B, R = px.shape[0], cfg.sp_resize_input
        dims = cfg.convnext_dims
        e = lambda *shape, dtype=F16: torch.empty(*shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            H = R // 4
            M = B * H * H
            patches = ops.sp_stem_patchify(px, R, e(M, 64))
            x = ops.gemm(patches, P["stem.w"], e(M, dims[0], dtype=F32), P["stem.b"], EPI_BIAS)
            ops.sp_layernorm(x, P["stem.ln"][0], P["stem.ln"][1], x)
            for i in range(4):
                C = dims[i]
                if i > 0:
                    rows = ops.sp_down_gather(x, P[f"down.{i}.ln"][0], P[f"down.{i}.ln"][1], B, H, H, e(M // 4, 4 * dims[i - 1]))
                    H, M = H // 2, M // 4
                    x = ops.gemm(rows, P[f"down.{i}.w"], e(M, C, dtype=F32), P[f"down.{i}.b"], EPI_BIAS)
                if not P["stages"][i]:
                    continue
                y, n, ff = e(M, C, dtype=F32), e(M, pad64(C)), e(M, 4 * C)
                for L in P["stages"][i]:
                    ops.sp_dwconv_ln(x, L["dw"], L["dwb"], L["ln"][0], L["ln"][1], B, H, H, n)
                    ops.gemm(n, L["w1"], ff, L["b1"], EPI_BIAS)
                    ops.sp_gelu(ff, ff)
                    ops.gemm(ff, L["w2"], y, L["b2"], EPI_RES, res=x)
                    x, y = y, x
        return x

    @torch.no_grad()
    def null_tokens(self) -> torch.Tensor:
        """fp32 [1, T, out_dim]: the tokens of the null input (a zero map with mask 0), ``linears(null_feature + pos_embedding)`` whatever the
        image; computed once per model and cached"""
        if self._null is None:
            from . import ops
            dev, T, C = self.device, self.T, self.cfg.convnext_dims[3]
            with torch.cuda.device(dev):
                a = ops.sp_assemble(torch.zeros(T, C, dtype=F32, device=dev), torch.zeros(1, dtype=F32, device=dev), self.P["null"], self.P["pos"],
                                    1, T, torch.empty(T, C, dtype=F16, device=dev))
                self._null = self._linears(a).view(1, T, self.D)
        return self._null

    @torch.no_grad()
    def tokens(self, map_: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """map fp32 [B, 3, S, S] in [-1, 1], mask [B] or [B, 1] -> grounding tokens fp32 [B, T, out_dim].  A sample with mask 0 gets the
        cached null tokens themselves (its features are multiplied by zero in the reference as well)."""
        from . import ops
        dev, T = self.device, self.T
        m = torch.as_tensor(mask).to(dev, F32).reshape(-1).contiguous()
        B = int(torch.as_tensor(map_).shape[0])
        if m.numel() != B:
            raise ValueError(f"mask has {m.numel()} entries for a batch of {B}")
        if not bool((m != 0).any()):          # the null input (one small read-back per image): no backbone run at all
            return self.null_tokens().expand(B, -1, -1).contiguous()
        feat = self.features(map_)
        with torch.cuda.device(dev):
            a = ops.sp_assemble(feat, m, self.P["null"], self.P["pos"], B, T, torch.empty(B * T, feat.shape[1], dtype=F16, device=dev))
            out = self._linears(a).view(B, T, self.D)
        return torch.where((m == 0).view(B, 1, 1), self.null_tokens(), out)


class SpatialDownsampler:
    def __init__(self, state_dict: Mapping[str, object], cfg: UNetConfig, device="cuda:0"):
        """``state_dict``: the checkpoint's ``model`` dict (``downsample_net.layers.*``; the hed family has no parameters)."""
        if not torch.cuda.is_available():
            raise RuntimeError("SpatialDownsampler needs a GPU: the downsampler has no CPU fallback")
        if cfg.ds_kind not in ("conv", "bicubic"):
            raise ValueError(f"ds_kind = {cfg.ds_kind!r}: the config has no grounding downsampler")
        self.cfg, self.device = cfg, torch.device(device)
        self.w = {}
        if cfg.ds_kind == "conv":
            for k, shp in (("layers.0.weight", (4, cfg.ds_in, 4, 4)), ("layers.0.bias", (4,)), ("layers.2.weight", (cfg.ds_out, 4, 4, 4)),
                           ("layers.2.bias", (cfg.ds_out,))):
                name = "downsample_net." + k
                if name not in state_dict:
                    raise KeyError(f"spatial checkpoint is missing {name}")
                t = torch.as_tensor(state_dict[name]).detach().to(self.device, F32).contiguous()
                if tuple(t.shape) != shp:
                    raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {shp}")
                self.w[k] = t
        self._tables: Dict[tuple, tuple] = {}

    @property
    def out_side(self) -> int:
        return self.cfg.ds_latent

    def _table(self, n_in: int, n_out: int):
        t = self._tables.get((n_in, n_out))
        if t is None:
            idx, w = bicubic_table(n_in, n_out)
            t = (torch.from_numpy(idx).to(self.device).contiguous(), torch.from_numpy(w).to(self.device).contiguous())
            self._tables[(n_in, n_out)] = t
        return t

    @torch.no_grad()
    def __call__(self, extra: torch.Tensor) -> torch.Tensor:
        """grounding_extra_input fp32 [B, 3, S, S'] -> fp32 [B, ds_out, side, side], side = resize_input / 4 (hed: 64)"""
        from . import ops
        cfg, dev = self.cfg, self.device
        x = torch.as_tensor(extra).to(dev, F32).contiguous()
        if x.dim() != 4 or x.shape[1] < cfg.ds_in:
            raise ValueError(f"grounding_extra_input {tuple(x.shape)}: need [B, >= {cfg.ds_in}, H, W]")
        B = x.shape[0]
        R = HED_DS_SIZE if cfg.ds_kind == "bicubic" else cfg.ds_resize_input
        e = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)
        with torch.cuda.device(dev):
            iy, wy = self._table(x.shape[2], R)
            ix, wx = self._table(x.shape[3], R)
            r = ops.sp_bicubic(x, cfg.ds_in, iy, wy, ix, wx, e(B, cfg.ds_in, R, R))
            if cfg.ds_kind == "bicubic":
                return r
            h = ops.sp_conv4x4s2(r, self.w["layers.0.weight"], self.w["layers.0.bias"], True, e(B, 4, R // 2, R // 2))
            return ops.sp_conv4x4s2(h, self.w["layers.2.weight"], self.w["layers.2.bias"], False, e(B, cfg.ds_out, R // 4, R // 4))


def map_stages(state_dict, cfg: UNetConfig, device):
    """(tokenizer, downsampler) of a map family, the two stages in front of the UNet.  The semantic-map family's both read one class map (a
    float one-hot is converted once for the two)."""
    if cfg.ds_kind == "sem":
        from .semantic import ClassMapInput, SemDownsampler, SemTokenizer
        cm = ClassMapInput(cfg.sem_classes, device)
        return SemTokenizer(state_dict, cfg, device, cm), SemDownsampler(state_dict, cfg, device, cm)
    return SpatialTokenizer(state_dict, cfg, device), SpatialDownsampler(state_dict, cfg, device)
