"""The front end of the semantic-map grounding family (GLIGEN's ``checkpoint_generation_sem.pth``) on the MI355X kernels of csrc/sem.hip; on
the engine such a model is an ordinary spatial handle (tokens through ``set_conditioning_tokens``, 8 channels through ``set_grounding_extra``).

The reference turns a 512 x 512 class map into a fp32 one-hot tensor [B, 152, 512, 512] (159 MB per sample), resizes it (nearest) and convolves
it twice: 152 -> 3 at 3x3 in ``sem_grounding_net.PositionNet.in_conv`` and 152 -> 16 at 4x4 stride 2 in ``sem_grounding_downsampler``.  A
convolution over a one-hot input is a table lookup, so both stages here read the uint8 CLASS MAP [B, H, W] (256 KB) and gather weights
(``gl_sem_gather_conv``); the one-hot tensor is never built on this path.

``SemTokenizer`` is ``sem_grounding_net.PositionNet``: class map -> in_conv by gather -> the ConvNeXt tokenizer of spatial.py from its stem on.
``SemDownsampler`` is ``sem_grounding_downsampler.GroundingDownsampler``: class map -> gather conv + SiLU -> ``gl_sem_conv4x4s2``.  Both also
take the reference's own float one-hot [B, C, H, W], converted once per ``sample()`` by ``gl_sem_onehot_index`` (``ClassMapInput``); a sample
that is not exactly one-hot is refused (a dense tensor is a different computation), unless its mask is 0.

No fallback: a missing GPU / library raises.
"""
from __future__ import annotations

import weakref
from typing import Mapping, Optional

import torch

from .arch import SEM_DS_HIDDEN, UNetConfig
from .spatial import SpatialTokenizer

F32 = torch.float32


def gather_table(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [Co, C, K, K] -> the gather table fp32 [C, K * K, Co padded to a multiple of 4] of gl_sem_gather_conv: one tap of one class
    is one contiguous row, the pad columns zero"""
    Co, C, K, _ = w.shape
    t = w.permute(1, 2, 3, 0).reshape(C, K * K, Co)
    return torch.nn.functional.pad(t, (0, (Co + 3) // 4 * 4 - Co)).to(F32).contiguous()


def _param(sd: Mapping[str, object], name: str, shape, device) -> torch.Tensor:
    if name not in sd:
        raise KeyError(f"spatial checkpoint is missing {name}")
    t = torch.as_tensor(sd[name]).detach().to(device, F32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {tuple(shape)}")
    return t


class ClassMapInput:
    """Either input form -> the uint8 class map [B, H, W] on the device.  An integer class map [B, H, W] (the native form) is checked against
    the class count; a float one-hot [B, C, H, W] is converted by gl_sem_onehot_index, sample by sample: a sample whose mask is 0 is neither
    converted nor validated (its map is class 0 throughout and its tokens are the null tokens), any other sample with a pixel that is not
    exactly one-hot raises ValueError naming it.  The last conversion is kept, so the tokenizer and the downsampler of one model, given the
    same tensor object, convert it once."""

    def __init__(self, classes: int, device):
        self.classes, self.device = int(classes), torch.device(device)
        self._last = None          # (weak reference to the tensor, its version, the samples converted, the class map)

    @torch.no_grad()
    def __call__(self, sem, mask=None) -> torch.Tensor:
        from . import ops
        x = torch.as_tensor(sem)
        dev, C = self.device, self.classes
        keep = list(range(x.shape[0])) if x.dim() else []
        if mask is not None and x.dim() == 4:
            m = torch.as_tensor(mask).reshape(-1)
            if m.numel() != x.shape[0]:
                raise ValueError(f"mask has {m.numel()} entries for a batch of {x.shape[0]}")
            keep = [b for b in keep if float(m[b]) != 0.0]
        if self._last is not None and self._last[0]() is x and self._last[1] == x._version and set(keep) <= self._last[2]:
            return self._last[3]
        if x.dim() == 3 and not x.is_floating_point() and x.dtype != torch.bool:
            hi = int(x.max()) if x.numel() else 0
            if hi >= C or (x.dtype != torch.uint8 and int(x.min()) < 0):
                raise ValueError(f"class map holds the value {hi if hi >= C else int(x.min())}: the model has the classes 0 .. {C - 1}")
            cm = x.to(dev, torch.uint8).contiguous()
        elif x.dim() == 4 and x.is_floating_point():
            if x.shape[1] != C:
                raise ValueError(f"one-hot sem {tuple(x.shape)}: the model has {C} classes, need [B, {C}, H, W]")
            B = x.shape[0]
            cm = torch.zeros(B, x.shape[2], x.shape[3], dtype=torch.uint8, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                for b in keep:
                    ops.sem_onehot_index(x[b:b + 1].to(dev, F32).contiguous(), cm[b:b + 1], bad[b:b + 1])
            if keep:
                counts = bad.cpu().tolist()
                wrong = [b for b in keep if counts[b]]
                if wrong:
                    raise ValueError(f"sem sample {wrong[0]} is not one-hot: {counts[wrong[0]]} of its pixels do not have exactly one channel at 1.0 "
                                     "and every other at 0.0 (a dense tensor is a different computation; pass a class map or a one-hot)")
        else:
            raise ValueError(f"sem {tuple(x.shape)} {x.dtype}: need an integer class map [B, H, W] or a float one-hot [B, {C}, H, W]")
        self._last = (weakref.ref(x), x._version, set(keep), cm)
        return cm


class SemTokenizer(SpatialTokenizer):
    def __init__(self, state_dict: Mapping[str, object], cfg: UNetConfig, device="cuda:0", class_map: Optional[ClassMapInput] = None):
        """``state_dict``: the checkpoint's ``model`` dict (``position_net.*`` names, ``position_net.in_conv.*`` among them)."""
        if cfg.ds_kind != "sem":
            raise ValueError(f"ds_kind = {cfg.ds_kind!r}: SemTokenizer belongs to the semantic-map family")
        super().__init__(state_dict, cfg, device)          # (pack_tokenizer has checked that in_conv.* are there, with their shapes)
        w = _param(state_dict, "position_net.in_conv.weight", (3, cfg.sem_classes, 3, 3), self.device)
        self.P["in_conv.table"] = gather_table(w)
        self.P["in_conv.b"] = _param(state_dict, "position_net.in_conv.bias", (3,), self.device)
        self.class_map = class_map if class_map is not None else ClassMapInput(cfg.sem_classes, self.device)

    @torch.no_grad()
    def in_conv(self, cmap: torch.Tensor) -> torch.Tensor:
        """uint8 class map [B, H, W] -> F.interpolate(onehot, R) -> in_conv -> fp32 [B, 3, R, R]"""
        from . import ops
        R = self.cfg.sp_resize_input
        with torch.cuda.device(self.device):
            return ops.sem_gather_conv(cmap, R, self.P["in_conv.table"], self.P["in_conv.b"], 3, 1, 1, False,
                                       torch.empty(cmap.shape[0], 3, R, R, dtype=F32, device=self.device))

    @torch.no_grad()
    def features(self, cmap: torch.Tensor) -> torch.Tensor:
        """uint8 class map [B, H, W] -> fp32 rows [B * T, dims[3]]: in_conv by gather, then the ConvNeXt from its stem on (the stem's nearest
        resize from R to R is the identity)"""
        return super().features(self.in_conv(cmap))

    @torch.no_grad()
    def tokens(self, sem, mask: torch.Tensor) -> torch.Tensor:
        """sem: class map [B, H, W] or float one-hot [B, C, H, W]; mask [B] or [B, 1] -> grounding tokens fp32 [B, T, out_dim]"""
        return super().tokens(self.class_map(sem, mask), mask)


class SemDownsampler:
    def __init__(self, state_dict: Mapping[str, object], cfg: UNetConfig, device="cuda:0", class_map: Optional[ClassMapInput] = None):
        """``state_dict``: the checkpoint's ``model`` dict (``downsample_net.layers.*``)."""
        if not torch.cuda.is_available():
            raise RuntimeError("SemDownsampler needs a GPU: the downsampler has no CPU fallback")
        if cfg.ds_kind != "sem":
            raise ValueError(f"ds_kind = {cfg.ds_kind!r}: SemDownsampler belongs to the semantic-map family")
        self.cfg, self.device = cfg, torch.device(device)
        C, Hd = cfg.sem_classes, SEM_DS_HIDDEN
        self.table = gather_table(_param(state_dict, "downsample_net.layers.0.weight", (Hd, C, 4, 4), self.device))
        self.b0 = _param(state_dict, "downsample_net.layers.0.bias", (Hd,), self.device)
        self.w2 = _param(state_dict, "downsample_net.layers.2.weight", (cfg.ds_out, Hd, 4, 4), self.device)
        self.b2 = _param(state_dict, "downsample_net.layers.2.bias", (cfg.ds_out,), self.device)
        self.class_map = class_map if class_map is not None else ClassMapInput(C, self.device)

    @property
    def out_side(self) -> int:
        return self.cfg.ds_latent

    @torch.no_grad()
    def __call__(self, extra) -> torch.Tensor:
        """grounding_extra_input (class map [B, H, W] or float one-hot [B, C, H, W]) -> fp32 [B, ds_out, R / 4, R / 4], R = resize_input"""
        from . import ops
        cfg, dev = self.cfg, self.device
        cm = self.class_map(extra)
        B, R = cm.shape[0], cfg.ds_resize_input
        e = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)
        with torch.cuda.device(dev):
            h = ops.sem_gather_conv(cm, R, self.table, self.b0, 4, 2, 1, True, e(B, SEM_DS_HIDDEN, R // 2, R // 2))
            return ops.sem_conv4x4s2(h, self.w2, self.b2, e(B, cfg.ds_out, R // 4, R // 4))
