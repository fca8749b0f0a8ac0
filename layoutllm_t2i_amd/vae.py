"""VAE decode stage on the HIP kernels (the first "next" row after the denoiser).

Replaces ``AutoencoderKL.decode`` (GLIGEN/ldm/models/autoencoder.py:40-44) and ``Decoder.forward``
(GLIGEN/ldm/modules/diffusionmodules/model.py:535-568): 1/scale_factor, 1x1 post_quant_conv, conv_in,
mid (ResnetBlock, single-head AttnBlock, ResnetBlock), 4 up levels x 3 ResnetBlocks with nearest-2x
upsample + conv, GroupNorm(eps 1e-6) + swish + conv_out.  2.5 TFLOP per 512x512 image.

No new heavy kernels: every conv / 1x1 conv / GroupNorm+swish goes through the denoiser's
``gl_conv3x3`` / ``gl_gemm`` / ``gl_groupnorm_*`` (NHWC fp16, fp32 accumulate).  The mid attention has one
head of d = 512, beyond the flash kernel's register budget; it runs once per image as
Q.K^T (GEMM) -> row softmax -> P.V (GEMM against V^T), with 1/sqrt(C) folded into the q weights at
pack time so the fp16 logits stay small.

``VAEEncoder.encode(x)`` is AutoencoderKL.encode (autoencoder.py:34-38): Encoder.forward (model.py:368-459), quant_conv, the
posterior sample and * scale_factor, through ``gl_vae_encoder_create`` / ``gl_vae_encode`` on the same engine (the stride-2
Downsample with its asymmetric F.pad(x, (0, 1, 0, 1)) is ``gl_conv3x3_pad01``, quant_conv + posterior one fp32 kernel,
``gl_vae_posterior``); ``encode_oplevel`` is its op-by-op test mirror.  ``VAEDecoder.encode`` delegates to an encoder built from
the same state dict when it holds the encoder tensors (real GLIGEN checkpoints do).

``VAEDecoder.decode(z)`` has the reference's contract: z fp32 [B, 4, h, w] -> fp32 [B, 3, 8h, 8w].  It is a thin caller
of the C engine (``gl_vae_create`` / ``gl_vae_load_weights`` / ``gl_vae_decode``, csrc/vae_engine.hip: plan, flat weight
layout, activation pool, one hipGraph per (batch, h, w)); ``decode_oplevel`` is the same launch sequence issued op by op
from Python -- the test mirror the C engine must equal bitwise, like tests/engine_pyref.py for the UNet.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Tuple

import torch

from . import ops
from ._lib import EPI_BIAS, EPI_RES, init_device
from .arch import VAEConfig, vae_decoder_param_shapes, vae_encoder_param_shapes
from .weights import CIN_PAD, _h, _t, copy_packed, flat_views, pack_conv3x3, pack_conv_upfold

F16, F32 = torch.float16, torch.float32
_FP32_1X1 = ("post_quant_conv", "quant_conv")      # 1x1 convs on the 4 / 8-channel latent side: kept in fp32


def _pack_kind(p: str, shp: Tuple[int, ...]) -> str:
    if len(shp) == 1:
        return "norm"                               # GroupNorm affine
    if shp[2] == 3:
        return "conv3x3"
    return "f32_1x1" if p in _FP32_1X1 else "gemm"


# narrowest upsample conv (channels) of a decoder whose up convs are folded under the default of option key 55 (2): the full decoder's 256- and
# 512-channel layers run in 0.46-0.54 of the 9-tap time at B = 4 (-1.6 ms per decode); a test-size decoder (128 channels, -7 us) keeps its pack
# unless fold_up=True or key 55 = 1 asks for the fold (profiles/upfold_shapes.txt)
VAE_UPFOLD_MIN_CHANNELS = 256


def _fold(fold_up, cfg) -> bool:
    from . import _lib
    ups = [shp[0] for n, shp in vae_decoder_param_shapes(cfg).items() if n.endswith(".upsample.conv.weight")]
    return _lib.resolve_fold_up(fold_up, bool(ups) and min(ups) >= VAE_UPFOLD_MIN_CHANNELS)


def _is_upsample(p: str) -> bool:
    return p.startswith("decoder.up.") and p.endswith(".upsample.conv")


def packed_shapes(param_shapes: Mapping[str, Tuple[int, ...]], fold_up: bool = False) -> Dict[str, Tuple[Tuple[int, ...], torch.dtype]]:
    """CPU-side: the engine-table entries {name: (shape, dtype)} the packer makes from reference-named ``param_shapes``
    (3x3 convs fp16 [Cout, 9 * Cin] with Cin < 64 padded to CIN_PAD, 1x1 convs fp16 [N, K] except the fp32 (post_)quant_conv,
    norm affine and biases fp32; with ``fold_up`` (a handle created under option key 55 = 1) the decoder's upsample convs fp16
    [4 * Cout, 4 * Cin])."""
    fold = bool(fold_up)
    out: Dict[str, Tuple[Tuple[int, ...], torch.dtype]] = {}
    for name, shp in param_shapes.items():
        if not name.endswith(".weight"):
            continue
        p, kind = name[:-7], _pack_kind(name[:-7], shp)
        if kind == "norm":
            out[p + ".g"], out[p + ".b"] = ((shp[0],), F32), ((shp[0],), F32)
            continue
        if kind == "conv3x3" and fold and _is_upsample(p):
            out[p + ".w"] = ((4 * shp[0], 4 * shp[1]), F16)
        elif kind == "conv3x3":
            out[p + ".w"] = ((shp[0], 9 * (CIN_PAD if shp[1] < 64 else shp[1])), F16)
        else:
            out[p + ".w"] = ((shp[0], shp[1]), F32 if kind == "f32_1x1" else F16)
        out[p + ".b"] = ((shp[0],), F32)
    return out


def _pack(state_dict: Mapping[str, object], need: Mapping[str, Tuple[int, ...]], device, fold_up=False) -> Dict[str, torch.Tensor]:
    """Reference-named tensors -> the engine's packed forms (``packed_shapes``); C^-0.5 folded into mid.attn_1.q; with ``fold_up`` the
    decoder's upsample convs as folded 2x2 kernels (weights.pack_conv_upfold)."""
    g = lambda k: _t(state_dict[k], device)
    W: Dict[str, torch.Tensor] = {}
    for name, shp in need.items():
        if not name.endswith(".weight"):
            continue
        p = name[:-7]
        w = g(name)
        b = g(p + ".bias")
        kind = _pack_kind(p, shp)
        if kind == "norm":
            W[p + ".g"], W[p + ".b"] = w.contiguous(), b.contiguous()
        elif kind == "conv3x3" and fold_up and _is_upsample(p):
            W[p + ".w"] = pack_conv_upfold(w)
            W[p + ".b"] = b.contiguous()
        elif kind == "conv3x3":
            W[p + ".w"] = pack_conv3x3(w, CIN_PAD if shp[1] < 64 else None)
            W[p + ".b"] = b.contiguous()
        elif kind == "f32_1x1":                     # 1x1 on the latent side: applied in fp32 (latent packing / posterior kernel)
            W[p + ".w"], W[p + ".b"] = w.reshape(shp[0], shp[1]).contiguous(), b.contiguous()
        else:                                       # 1x1 conv = GEMM
            w2, b2 = w.reshape(shp[0], shp[1]), b
            if p.endswith("attn_1.q"):              # fold the softmax scale C^-0.5 (model.py:183) into q
                s = float(shp[0]) ** -0.5
                w2, b2 = w2 * s, b2 * s
            W[p + ".w"], W[p + ".b"] = _h(w2), b2.contiguous()
    return W


def encoder_unsupported(state_dict: Mapping[str, object], cfg: VAEConfig):
    """Why this package cannot run the checkpoint's encoder (down-level attention, in_channels != out_ch), or None."""
    attn = sorted(k for k in state_dict if k.startswith("encoder.down.") and ".attn." in k)
    if attn:
        return f"the VAE encoder has down-level attention ({attn[0]}); only attn_resolutions = [] is implemented"
    w = state_dict.get("encoder.conv_in.weight")
    if w is not None and tuple(w.shape)[1] != cfg.out_ch:
        return f"the VAE encoder takes {tuple(w.shape)[1]} input channels, the decoder emits out_ch = {cfg.out_ch}"
    return None


class _VAEStage:
    """Engine binding, option knob, pooled buffers and the ResnetBlock / AttnBlock op sequences shared by both stages."""
    _encoder_stage = False

    def _bind_engine(self):
        """Moves the packed tensors into the C engine's flat layout (gl_vae_weight_at) and rebinds ``W`` to views of it."""
        from . import _lib
        self.handle = _lib.create_vae(self.cfg, encoder=self._encoder_stage, fold_up=getattr(self, "fold_up", None))
        flat, views = flat_views(*_lib.vae_weight_table(self.handle), self.device)
        for name, dst in views.items():
            copy_packed(name, dst, self.W[name])
        extra = set(self.W) - set(views)
        if extra:
            raise KeyError(f"packer produced tensors the VAE engine does not know: {sorted(extra)[:3]}")
        self.W, self.flat = views, flat
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gl_vae_load_weights(self.handle, flat.data_ptr(), flat.numel(), torch.cuda.current_stream(self.device).cuda_stream),
                       "gl_vae_load_weights")
        self.use_graphs = True

    def set_option(self, key: int, value: int) -> None:
        """Override one gl_set_option knob for THIS stage only (gl_vae_set_option)."""
        from . import _lib
        _lib.check(_lib.lib().gl_vae_set_option(self.handle, int(key), int(value)), "gl_vae_set_option")

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                from . import _lib
                _lib.lib().gl_vae_destroy(h)
            except Exception:
                pass

    def buf(self, tag, shape, dtype=F16):
        key = (tag, tuple(shape), dtype)
        t = self._pool.get(key)
        if t is None:
            t = torch.empty(tuple(shape), dtype=dtype, device=self.device)
            self._pool[key] = t
        return t

    # ---- blocks
    def _gn(self, x, B, HW, p, silu, tag):
        C = x.shape[-1]
        nchunk = ops.gn_nchunk(HW)
        partial = self.buf("gn.partial", (B * nchunk * 64,), F32)
        return ops.groupnorm(x, None, B, HW, self.W[p + ".g"], self.W[p + ".b"], 1e-6, silu, self.buf(tag, (B * HW, C)), partial)

    def _resnet(self, p, x, B, sh, sw, cin, cout, tag):
        W, HW, side = self.W, sh * sw, f"{sh}x{sw}"
        t = self._gn(x, B, HW, p + ".norm1", True, f"rn.gn.{cin}.{side}")
        h = ops.conv3x3(t, W[p + ".conv1.w"], self.buf(f"rn.h.{cout}.{side}", (B * HW, cout)), B, sh, sw, W[p + ".conv1.b"])
        t2 = self._gn(h, B, HW, p + ".norm2", True, f"rn.gn.{cout}.{side}")
        if cin != cout:
            sk = ops.gemm(x, W[p + ".nin_shortcut.w"], self.buf(f"rn.sk.{cout}.{side}", (B * HW, cout)), W[p + ".nin_shortcut.b"])
        else:
            sk = x
        return ops.conv3x3(t2, W[p + ".conv2.w"], self.buf(tag, (B * HW, cout)), B, sh, sw, W[p + ".conv2.b"],
                           epi=EPI_RES, res=sk)

    def _attn(self, p, x, B, N, C, tag):
        W = self.W
        M = B * N
        hn = self._gn(x, B, N, p + ".norm", False, "at.gn")
        q = ops.gemm(hn, W[p + ".q.w"], self.buf("at.q", (M, C)), W[p + ".q.b"])
        k = ops.gemm(hn, W[p + ".k.w"], self.buf("at.k", (M, C)), W[p + ".k.b"])
        v = ops.gemm(hn, W[p + ".v.w"], self.buf("at.v", (M, C)), W[p + ".v.b"])
        Np = (N + 63) // 64 * 64
        Hs = 4                                              # split C only for the transpose kernel's tile
        vt = self.buf("at.vt", (B, Hs, C // Hs, Np))
        ops.transpose_v(v, N * C, C, vt, B, Hs, C // Hs, N)
        vt2 = vt.view(B, C, Np)
        s = self.buf("at.s", (B, N, Np))
        if Np != N:
            s.zero_()
        o = self.buf("at.o", (M, C))
        for b in range(B):
            sb = s[b][:, :N]
            ops.gemm(q[b * N:(b + 1) * N], k[b * N:(b + 1) * N], sb)      # logits already carry C^-0.5
            ops.softmax_rows(sb, 1.0)
            ops.gemm(s[b], vt2[b], o[b * N:(b + 1) * N])                  # P [N, Np] . V^T[C, Np]^T
        return ops.gemm(o, W[p + ".proj_out.w"], self.buf(tag, (M, C)), W[p + ".proj_out.b"], EPI_RES, res=x)


class VAEDecoder(_VAEStage):
    def __init__(self, state_dict: Mapping[str, object], cfg: VAEConfig = VAEConfig(), device="cuda:0", fold_up=None):
        """``fold_up``: the upsample convs as folded 2x2 kernels (None: the current value of option key 55, whose default folds decoders
        whose up convs have at least VAE_UPFOLD_MIN_CHANNELS channels)."""
        if not torch.cuda.is_available():
            raise RuntimeError("VAEDecoder needs a GPU: there is no CPU fallback")
        init_device()
        self.cfg, self.device = cfg, torch.device(device)
        self.scale_factor = cfg.scale_factor
        self.fold_up = _fold(fold_up, cfg)
        need = vae_decoder_param_shapes(cfg)
        missing = [k for k in need if k not in state_dict]
        if missing:
            raise KeyError(f"autoencoder state_dict is missing {len(missing)} decoder tensors, e.g. {missing[:3]}")
        self.W = _pack(state_dict, need, self.device, self.fold_up)
        self._pool: Dict[tuple, torch.Tensor] = {}
        self._bind_engine()
        # the encode stage, when the state dict carries it (real GLIGEN checkpoints do); self.W stays decoder-only
        enc_missing = [k for k in vae_encoder_param_shapes(cfg) if k not in state_dict]
        self.encoder = VAEEncoder(state_dict, cfg, device) if not enc_missing else None
        self._no_encoder = (f"this autoencoder has no encode stage: its state_dict lacks {len(enc_missing)} encoder tensors, "
                            f"e.g. {enc_missing[:3]}") if enc_missing else None

    @classmethod
    def from_packed(cls, W: Mapping[str, torch.Tensor], cfg: VAEConfig, device="cuda:0") -> "VAEDecoder":
        """A decoder around ALREADY PACKED tensors (``self.W`` of another instance, e.g. received through
        dist.broadcast_bundle): no state_dict, no repacking."""
        if not torch.cuda.is_available():
            raise RuntimeError("VAEDecoder needs a GPU: there is no CPU fallback")
        init_device()
        self = cls.__new__(cls)
        self.cfg, self.device, self.scale_factor = cfg, torch.device(device), cfg.scale_factor
        self.W = {k: v.to(self.device) for k, v in W.items()}
        # folded or 9-tap upsample convs: what the packed tensors are ([4 C, 4 C] against [C, 9 C])
        ups = [v for k, v in self.W.items() if k.endswith(".w") and _is_upsample(k[:-2])]
        self.fold_up = bool(ups) and all(v.shape[0] == v.shape[1] for v in ups)
        self._pool = {}
        self._bind_engine()
        self.encoder = None
        self._no_encoder = ("this decoder was built from packed decoder weights: the encoder tensors (encoder.*, quant_conv.*) are "
                            "not part of the packed bundle")
        return self

    def encode(self, x: torch.Tensor, noise=None) -> torch.Tensor:
        """AutoencoderKL.encode (autoencoder.py:34-38) through the encoder built from the same state dict."""
        if self.encoder is None:
            raise RuntimeError(self._no_encoder)
        return self.encoder.encode(x, noise)

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """AutoencoderKL.decode through the C engine (one hipGraph replay per call after the first)."""
        from . import _lib
        cfg = self.cfg
        z = z.to(self.device, F32).contiguous()
        B, zc, sh, sw = z.shape
        assert zc == cfg.z_channels
        f = 2 ** (len(cfg.ch_mult) - 1)
        out = torch.empty(B, cfg.out_ch, f * sh, f * sw, dtype=F32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if sh == sw:
                _lib.check(_lib.lib().gl_vae_decode(self.handle, z.data_ptr(), B, sh, out.data_ptr(), int(self.use_graphs), st), "gl_vae_decode")
            else:
                _lib.check(_lib.lib().gl_vae_decode_hw(self.handle, z.data_ptr(), B, sh, sw, out.data_ptr(), int(self.use_graphs), st),
                           "gl_vae_decode_hw")
        return out

    @torch.no_grad()
    def decode_oplevel(self, z: torch.Tensor) -> torch.Tensor:
        """The engine's launch sequence issued op by op from Python (test mirror; bitwise equal to ``decode``)."""
        cfg, W = self.cfg, self.W
        z = z.to(self.device, F32).contiguous()
        B, zc, sh, sw = z.shape
        assert zc == cfg.z_channels
        nres = len(cfg.ch_mult)
        ch = cfg.ch * cfg.ch_mult[nres - 1]
        xin = ops.latent_affine_pack(z, W["post_quant_conv.w"], W["post_quant_conv.b"], 1.0 / cfg.scale_factor, CIN_PAD,
                                     self.buf("in", (B * sh * sw, CIN_PAD)))
        h = ops.conv3x3(xin, W["decoder.conv_in.w"], self.buf("conv_in", (B * sh * sw, ch)), B, sh, sw, W["decoder.conv_in.b"])
        h = self._resnet("decoder.mid.block_1", h, B, sh, sw, ch, ch, "mid.1")
        h = self._attn("decoder.mid.attn_1", h, B, sh * sw, ch, "mid.a")
        h = self._resnet("decoder.mid.block_2", h, B, sh, sw, ch, ch, "mid.2")
        for lvl in reversed(range(nres)):
            cout = cfg.ch * cfg.ch_mult[lvl]
            for i in range(cfg.num_res_blocks + 1):
                h = self._resnet(f"decoder.up.{lvl}.block.{i}", h, B, sh, sw, ch, cout, f"up.{lvl}.{i}")
                ch = cout
            if lvl != 0:
                p = f"decoder.up.{lvl}.upsample.conv"
                h = ops.conv3x3(h, W[p + ".w"], self.buf(f"up.{lvl}.u", (B * 4 * sh * sw, ch)), B, sh, sw, W[p + ".b"],
                                upsample2x=True)
                sh, sw = 2 * sh, 2 * sw
        g = self._gn(h, B, sh * sw, "decoder.norm_out", True, "fin.gn")
        out = torch.empty(B, cfg.out_ch, sh, sw, dtype=F32, device=self.device)
        ops.conv3x3(g, W["decoder.conv_out.w"], out, B, sh, sw, W["decoder.conv_out.b"], nchw_hw=sh * sw)
        return out


class VAEEncoder(_VAEStage):
    """AutoencoderKL.encode on the HIP engine: x fp32 [B, 3, H, W] in [-1, 1] -> z fp32 [B, embed_dim, H / f, W / f], f = 8."""
    _encoder_stage = True

    def __init__(self, state_dict: Mapping[str, object], cfg: VAEConfig = VAEConfig(), device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("VAEEncoder needs a GPU: there is no CPU fallback")
        why = encoder_unsupported(state_dict, cfg)
        if why:
            raise NotImplementedError(why)
        init_device()
        self.cfg, self.device = cfg, torch.device(device)
        self.scale_factor = cfg.scale_factor
        need = vae_encoder_param_shapes(cfg)
        missing = [k for k in need if k not in state_dict]
        if missing:
            raise KeyError(f"autoencoder state_dict is missing {len(missing)} encoder tensors, e.g. {missing[:3]}")
        self.W = _pack(state_dict, need, self.device)
        self._pool: Dict[tuple, torch.Tensor] = {}
        self._bind_engine()

    @property
    def factor(self) -> int:
        return 2 ** (len(self.cfg.ch_mult) - 1)

    def _check(self, x: torch.Tensor):
        x = x.to(self.device, F32).contiguous()
        if x.dim() != 4 or x.shape[1] != self.cfg.out_ch:
            raise ValueError(f"encode: expected a [B, {self.cfg.out_ch}, H, W] image batch, got {tuple(x.shape)}")
        B, c, sh, sw = x.shape
        f = self.factor
        for side in (sh, sw):
            if side % f or side >= 1024:
                raise ValueError(f"encode: the image's height and width must each be a multiple of {f} and below 1024, got {sh} x {sw}")
        return x, B, (sh, sw), (sh // f, sw // f)

    def _noise(self, noise, B, zs):
        shape = (B, self.cfg.embed_dim, *zs)
        if noise is None:   # distributions.py:36: torch.randn(mean.shape) on the CPU default generator, then moved to the device
            noise = torch.randn(shape)
        noise = noise.to(self.device, F32).contiguous()
        if tuple(noise.shape) != shape:
            raise ValueError(f"encode: noise must be {list(shape)}, got {tuple(noise.shape)}")
        return noise

    @torch.no_grad()
    def encode(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """posterior.sample() * scale_factor through the C engine (one hipGraph replay per call after the first)."""
        from . import _lib
        x, B, (sh, sw), zs = self._check(x)
        noise = self._noise(noise, B, zs)
        z = torch.empty(B, self.cfg.embed_dim, *zs, dtype=F32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if sh == sw:
                _lib.check(_lib.lib().gl_vae_encode(self.handle, x.data_ptr(), B, sh, noise.data_ptr(), z.data_ptr(), int(self.use_graphs), st),
                           "gl_vae_encode")
            else:
                _lib.check(_lib.lib().gl_vae_encode_hw(self.handle, x.data_ptr(), B, sh, sw, noise.data_ptr(), z.data_ptr(),
                                                       int(self.use_graphs), st), "gl_vae_encode_hw")
        return z

    @torch.no_grad()
    def encode_oplevel(self, x: torch.Tensor, noise: torch.Tensor, return_mean: bool = False):
        """The engine's launch sequence issued op by op from Python (test mirror; bitwise equal to ``encode``).
        ``return_mean``: also the posterior mean (unscaled)."""
        cfg, W = self.cfg, self.W
        x, B, (sh, sw), zs = self._check(x)
        noise = self._noise(noise, B, zs)
        nres = len(cfg.ch_mult)
        ch = cfg.ch
        xin = ops.pack_latent(x, CIN_PAD, 1, self.buf("in", (B * sh * sw, CIN_PAD)))
        h = ops.conv3x3(xin, W["encoder.conv_in.w"], self.buf("conv_in", (B * sh * sw, ch)), B, sh, sw, W["encoder.conv_in.b"])
        for lvl in range(nres):
            cout = cfg.ch * cfg.ch_mult[lvl]
            for i in range(cfg.num_res_blocks):
                h = self._resnet(f"encoder.down.{lvl}.block.{i}", h, B, sh, sw, ch, cout, f"down.{lvl}.{i}")
                ch = cout
            if lvl != nres - 1:
                p = f"encoder.down.{lvl}.downsample.conv"
                h = ops.conv3x3_pad01(h, W[p + ".w"], self.buf(f"down.{lvl}.d", (B * (sh // 2) * (sw // 2), ch)), B, sh, sw, W[p + ".b"])
                sh, sw = sh // 2, sw // 2
        h = self._resnet("encoder.mid.block_1", h, B, sh, sw, ch, ch, "mid.1")
        h = self._attn("encoder.mid.attn_1", h, B, sh * sw, ch, "mid.a")
        h = self._resnet("encoder.mid.block_2", h, B, sh, sw, ch, ch, "mid.2")
        g = self._gn(h, B, sh * sw, "encoder.norm_out", True, "fin.gn")
        mom = torch.empty(B, 2 * cfg.z_channels, sh, sw, dtype=F32, device=self.device)
        ops.conv3x3(g, W["encoder.conv_out.w"], mom, B, sh, sw, W["encoder.conv_out.b"], nchw_hw=sh * sw)
        z = torch.empty(B, cfg.embed_dim, sh, sw, dtype=F32, device=self.device)
        mean = torch.empty_like(z) if return_mean else None
        ops.vae_posterior(mom, W["quant_conv.w"], W["quant_conv.b"], noise, cfg.scale_factor, z, mean)
        return (z, mean) if return_mean else z
