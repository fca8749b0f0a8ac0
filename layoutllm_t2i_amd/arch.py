"""Static description of the layout-conditioned UNet: block plan and parameter table.

The reference builds its UNet imperatively inside ``UNetModel.__init__``
(GLIGEN/ldm/modules/diffusionmodules/openaimodel.py:234-391).  Here the same
topology is *derived as data*: a flat list of layer records that the HIP engine
walks, plus the table of state_dict names/shapes so that a
real GLIGEN checkpoint loads by name.

Nothing here touches a device.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Dict, List, Tuple


KEYPOINTS = 17           # COCO keypoints per person (keypoint_grounding_net.py:16)
MAX_PERSONS = 8          # the shipped checkpoint's max_persons_per_image: 136 grounding tokens (gl_create's limit for the family)

# The spatial grounding families: tokenizer module -> (its own downsampler module, downsampler kind, input channels, default output channels).
# {canny,hed,depth,normal}_grounding_net.PositionNet are one ConvNeXt tokenizer; *_grounding_downsampler.py differ in the channels they read and
# in whether two small convs follow the bicubic resize (hed: none, a hard-coded 64 x 64).  The semantic family (sem_grounding_net: a one-hot
# class-map input, nearest resize; from_dict(allow_semantic=True), semantic.py) is the same tokenizer behind an in_conv and is NOT in this table.
SPATIAL_FAMILIES = {
    "canny_grounding_net": ("canny_grounding_downsampler", "conv", 1, 8),
    "hed_grounding_net": ("hed_grounding_downsampler", "bicubic", 1, 1),
    "depth_grounding_net": ("depth_grounding_downsampler", "conv", 1, 8),
    "normal_grounding_net": ("normal_grounding_downsampler", "conv", 3, 8),
}
CONVNEXT_DEPTHS = (3, 3, 9, 3)            # convnext.py: convnext_tiny
CONVNEXT_DIMS = (96, 192, 384, 768)
HED_DS_SIZE = 64                          # hed_grounding_downsampler.py:19 resizes to (64, 64) whatever the latent
SEM_TOKENIZER = "sem_grounding_net.PositionNet"                                # the semantic-map family (checkpoint_generation_sem.pth)
SEM_DOWNSAMPLER = "sem_grounding_downsampler.GroundingDownsampler"
SEM_CLASSES = 152                         # configs/ade_sem.yaml: in_dim of both modules (150 ADE classes + 2)
SEM_DS_HIDDEN = 16                        # sem_grounding_downsampler.py:16: Conv2d(in_dim, 16, 4, 2, 1)


@dataclass(frozen=True)
class UNetConfig:
    """Hyper-parameters; defaults are GLIGEN/configs/coco2014.yaml:9-30."""
    image_size: int = 64
    in_channels: int = 4
    model_channels: int = 320
    out_channels: int = 4
    num_res_blocks: int = 2
    attention_resolutions: Tuple[int, ...] = (4, 2, 1)
    channel_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_heads: int = 8
    context_dim: int = 768
    pos_in_dim: int = 768        # PositionNet in_dim  (text_grounding_net.py:7)
    pos_out_dim: int = 768       # PositionNet out_dim
    fourier_freqs: int = 8
    max_objs: int = 30           # interface.py:158,425
    # not a hyper-parameter of the network: the packed-weight LAYOUT (gl_unet_config.split_weights).  True stores every matrix as
    # [Whi | Wlo] halves, which the engine's strict mode (option 50: split-fp16 operands, within north_star's tolerance of the fp32
    # reference) needs for its third pass; the default mode of such an engine reads the Whi halves.  Twice the weight bytes.
    split_weights: bool = False
    # the grounding tokenizer (config['model']['params']['grounding_tokenizer']['target']): "text" = text_grounding_net.PositionNet (one token
    # per box), "text_image" = text_image_grounding_net.PositionNet (GLIGEN's *_box_text_image checkpoints: a text token and an image token
    # per box, gl_unet_config.grounding = 1), "keypoint" = keypoint_grounding_net.PositionNet (checkpoint_generation_keypoint.pth: one token
    # per keypoint of up to max_persons people, 17 each, from 2-D points and two learned tables; gl_unet_config.grounding = 2; there max_objs
    # counts TOKENS, 17 * max_persons, and pos_in_dim is the person-feature width = pos_out_dim)
    grounding: str = "text"
    # GLIGEN's inpainting checkpoints (checkpoint_inpainting_text*.pth; openaimodel.py:293-299, :436-439): the first conv also reads the masked
    # image latent and the mask, cat([x, z0 * mask, mask]) -- in_channels stays the LATENT's channel count (gl_unet_config.inpaint_mode)
    inpaint_mode: bool = False
    # the transformer block: True = LayoutLLM-T2I's (attention.py:394-402, attn1 -> fuser -> rela_fuse -> attn2 -> ff); False = upstream GLIGEN's
    # (attention_original.py:312-316, no rela_fuse), what every public GLIGEN checkpoint was trained on (gl_unet_config.no_relation).  Not in
    # the config dict of a checkpoint: interface.load_ckpt sets it from the state dict's keys
    relation: bool = True
    # grounding = "spatial" (GLIGEN's canny / hed / depth / normal checkpoints, gl_unet_config.grounding = 4): a ConvNeXt tokenizer
    # (spatial.SpatialTokenizer: the map resized to sp_resize_input, (sp_resize_input // 32) ** 2 tokens) and a grounding downsampler whose
    # ds_out channels are concatenated to the latent in front of the first conv (spatial.SpatialDownsampler).  ds_kind: "" = none, "conv" =
    # bicubic to ds_resize_input then two 4x4 stride-2 convs (canny, depth, normal), "bicubic" = bicubic to 64 x 64 alone (hed); ds_in = the
    # channels of the map it reads (1, or 3 for normal).  The defaults leave every other config as it was.
    # ds_kind "sem" (the semantic-map family, also grounding = "spatial"): ds_in = the number of classes (the in_dim of the tokenizer's in_conv
    # and of the downsampler's first conv); nearest resize of the class map to ds_resize_input, Conv2d(ds_in, 16, 4, 2, 1), SiLU,
    # Conv2d(16, ds_out, 4, 2, 1) (semantic.SemDownsampler); the tokenizer is the ConvNeXt one behind in_conv (semantic.SemTokenizer).
    ds_kind: str = ""
    ds_in: int = 1
    ds_out: int = 0
    ds_resize_input: int = 256
    sp_resize_input: int = 256
    convnext_depths: Tuple[int, ...] = CONVNEXT_DEPTHS
    convnext_dims: Tuple[int, ...] = CONVNEXT_DIMS

    @property
    def first_conv_in(self) -> int:
        """input channels of input_blocks.0.0: the latent, plus the masked latent and the mask of an inpaint_mode model (4 + 4 + 1), or plus the
        grounding downsampler's channels of a spatial model (4 + 8, hed 4 + 1)"""
        return self.in_channels + (self.in_channels + 1 if self.inpaint_mode else self.ds_out)

    @property
    def n_ground(self) -> int:
        """grounding tokens per sample, the extra keys of the gated self-attention: max_objs (text, keypoint), 2 * max_objs (text_image) or the
        tokenizer's (sp_resize_input // 32) ** 2 (spatial)"""
        if self.grounding == "spatial":
            return (self.sp_resize_input // 32) ** 2
        return self.max_objs * (2 if self.grounding == "text_image" else 1)

    @property
    def sem_classes(self) -> int:
        """classes of a semantic-map model's class map (ds_in there), 0 on every other config"""
        return self.ds_in if self.ds_kind == "sem" else 0

    @property
    def ds_latent(self) -> int:
        """side of the downsampler's output, which the latent has to match: ds_resize_input / 4, or hed's hard-coded 64"""
        return HED_DS_SIZE if self.ds_kind == "bicubic" else self.ds_resize_input // 4

    @property
    def max_persons(self) -> int:
        """people per image of a keypoint model (keypoint_grounding_net.py:10): max_objs = 17 * max_persons tokens"""
        if self.grounding != "keypoint":
            raise AttributeError(f"max_persons: grounding = {self.grounding!r} has boxes, not persons")
        return self.max_objs // KEYPOINTS

    @property
    def time_embed_dim(self) -> int:
        return self.model_channels * 4

    @property
    def position_dim(self) -> int:
        """Fourier features of one location: sin & cos per frequency of the 4 box coordinates, or of the 2 of a keypoint"""
        return self.fourier_freqs * 2 * (2 if self.grounding == "keypoint" else 4)

    @staticmethod
    def from_dict(params: dict, allow_inpaint: bool = False, allow_keypoint: bool = False, allow_spatial: bool = False,
                  allow_semantic: bool = False) -> "UNetConfig":
        """Accepts the ``config['model']['params']`` dict of a GLIGEN checkpoint.

        ``allow_inpaint``: an ``inpaint_mode`` checkpoint (9-channel first conv) shares every parameter name with the layout-to-image UNet but
        needs ``inpainting_extra_input`` on every forward, so a caller has to say that it supplies one (``interface.load_ckpt`` does); without
        the flag such a config keeps raising, like the other look-alike variants below.

        ``allow_keypoint``: the same for a keypoint checkpoint (``keypoint_grounding_net.PositionNet``): it is fed ``points`` and ``masks``
        where the box families take boxes and embeddings, so a caller has to say that it supplies them (``interface.load_ckpt`` does).

        ``allow_spatial``: the same for the canny / hed / depth / normal checkpoints (``*_grounding_net.PositionNet`` with their own
        ``*_grounding_downsampler.GroundingDownsampler``): they are fed a map and ``grounding_extra_input``.  Every other downsampler config
        (no flag, another target, the sem family, with inpaint_mode, a tokenizer of another family) raises NotImplementedError naming
        ``grounding_downsampler``.

        ``allow_semantic``: the same for the semantic-map checkpoint (``sem_grounding_net.PositionNet`` with
        ``sem_grounding_downsampler.GroundingDownsampler``): it is fed a class map under the key ``sem``.  It reads as ``grounding ==
        "spatial"`` with ``ds_kind == "sem"`` and ``ds_in`` = the classes (both modules' ``in_dim``, which must agree, 2 .. 256); without the
        flag, or with the downsampler of another family, it raises NotImplementedError naming ``grounding_downsampler`` as before."""
        gt = (params.get("grounding_tokenizer") or {}).get("params", {})
        target = (params.get("grounding_tokenizer") or {}).get("target")
        if target is None or target.endswith(".text_grounding_net.PositionNet") or target == "text_grounding_net.PositionNet":
            grounding = "text"
        elif target.endswith("text_image_grounding_net.PositionNet"):
            grounding = "text_image"
        elif target.endswith("keypoint_grounding_net.PositionNet") and allow_keypoint:
            grounding = "keypoint"
        elif _spatial_family(target) is not None and allow_spatial and params.get("grounding_downsampler") is not None:
            grounding = "spatial"
        elif target.endswith(SEM_TOKENIZER) and allow_semantic and str((params.get("grounding_downsampler") or {}).get("target")).endswith(
                SEM_DOWNSAMPLER):
            grounding = "spatial"
        elif _spatial_family(target) is not None or target.endswith("sem_grounding_net.PositionNet"):
            raise NotImplementedError(f"grounding_tokenizer target {target!r} with grounding_downsampler "
                                      f"{(params.get('grounding_downsampler') or {}).get('target')!r}: the canny / hed / depth / normal families load "
                                      "with allow_spatial=True and their own grounding_downsampler (interface.load_ckpt passes the flag); the "
                                      "semantic family is not supported")
        else:
            raise NotImplementedError(f"grounding_tokenizer target {target!r}: only the text and text_image PositionNets are supported (and the "
                                      "keypoint one with allow_keypoint=True, fed points and masks: interface.load_ckpt / run_one_image do)")
        # variants that share parameter names / shapes with this UNet but compute something else must not load silently
        # (load_state_dict(strict=False), interface.py:91, would accept them): openaimodel.py:246-262, attention.py:362-384
        if params.get("fuser_type", "gatedSA") != "gatedSA":
            raise NotImplementedError(f"fuser_type={params.get('fuser_type')!r}: only 'gatedSA' is on the layout-to-image path")
        if int(params.get("transformer_depth", 1)) != 1:
            raise NotImplementedError("transformer_depth != 1 is not supported")
        if params.get("inpaint_mode", False) and params.get("grounding_downsampler") is not None:
            # (the reference itself stops at a breakpoint() there, openaimodel.py:437-438)
            raise NotImplementedError("grounding_downsampler with inpaint_mode is not supported (the reference stops there too)")
        if params.get("inpaint_mode", False) and not allow_inpaint:
            raise NotImplementedError("inpaint_mode checkpoints (9-channel first conv) are not on the layout-to-image path: pass "
                                      "allow_inpaint=True and feed inpainting_extra_input (interface.load_ckpt / run_one_image do)")
        sp = {}
        if params.get("grounding_downsampler") is not None:
            ds = params["grounding_downsampler"]
            ds_target, dp = str(ds.get("target")), ds.get("params") or {}
            if grounding != "spatial":
                raise NotImplementedError(f"grounding_downsampler {ds_target!r} is not on the text_layout path" +
                                          ("" if allow_spatial else " (the canny / hed / depth / normal families need allow_spatial=True)"))
            sem = target.endswith(SEM_TOKENIZER)
            if sem:
                # both in_dims are the number of classes; a uint8 class map holds up to 256
                cin, tin = int(dp.get("in_dim", SEM_CLASSES)), int(gt.get("in_dim", SEM_CLASSES))
                if cin != tin:
                    raise ValueError(f"sem grounding_tokenizer in_dim = {tin} but grounding_downsampler in_dim = {cin}: both are the number of classes")
                if not 2 <= cin <= 256:
                    raise ValueError(f"sem in_dim = {cin}: 2 .. 256 classes (the class map is uint8)")
                cout = int(dp.get("out_dim", 8))
                if not 1 <= cout <= 60:
                    raise ValueError(f"sem grounding_downsampler out_dim = {cout}: 1 .. 60")
                ds_mod, kind = "sem_grounding_downsampler", "sem"
            else:
                ds_mod, kind, cin, cout = SPATIAL_FAMILIES[_spatial_family(target)]
            if not ds_target.endswith(ds_mod + ".GroundingDownsampler"):
                raise NotImplementedError(f"grounding_downsampler target {ds_target!r} does not go with the tokenizer {target!r}: expected "
                                          f"{ds_mod}.GroundingDownsampler")
            if int(dp.get("out_dim", cout)) != cout:
                raise NotImplementedError(f"grounding_downsampler out_dim = {dp.get('out_dim')}: {ds_mod} has {cout}")
            sp = dict(ds_kind=kind, ds_in=cin, ds_out=cout, ds_resize_input=int(dp.get("resize_input", 256)),
                      sp_resize_input=int(gt.get("resize_input", 448)), relation=False)
            if sp["sp_resize_input"] % 32 or not 32 <= sp["sp_resize_input"] <= 256:
                raise ValueError(f"grounding_tokenizer resize_input = {sp['sp_resize_input']}: a multiple of 32 up to 256 (at most 64 grounding tokens)")
            if kind in ("conv", "sem") and (sp["ds_resize_input"] % 4 or sp["ds_resize_input"] <= 0):
                raise ValueError(f"grounding_downsampler resize_input = {sp['ds_resize_input']}: a multiple of 4")
            sp["max_objs"] = (sp["sp_resize_input"] // 32) ** 2
            if sem:
                sp["pos_in_dim"] = UNetConfig.pos_in_dim      # the tokenizer's in_dim counts classes there (ds_in), it is no embedding width
        if not params.get("use_spatial_transformer", True):
            raise NotImplementedError("use_spatial_transformer=False is not supported")
        kp = {}
        if grounding == "keypoint":
            if params.get("inpaint_mode", False):
                raise NotImplementedError("a keypoint grounding tokenizer with inpaint_mode: no such checkpoint exists, and the inpainting mask is "
                                          "drawn from boxes")
            if "max_persons_per_image" not in gt:
                raise ValueError("keypoint grounding_tokenizer params need max_persons_per_image")
            P = int(gt["max_persons_per_image"])
            if not 1 <= P <= MAX_PERSONS:
                raise ValueError(f"max_persons_per_image = {P}: 1 .. {MAX_PERSONS} are supported ({KEYPOINTS} grounding tokens per person)")
            # keypoint_grounding_net.py:10-31: one width, out_dim, for the person features and the tokens; 17 P tokens
            kp = dict(max_objs=KEYPOINTS * P, pos_in_dim=int(gt.get("out_dim", 768)), relation=False)
        cfg = UNetConfig(
            image_size=int(params.get("image_size", 64)),
            in_channels=int(params.get("in_channels", 4)),
            model_channels=int(params.get("model_channels", 320)),
            out_channels=int(params.get("out_channels", 4)),
            num_res_blocks=int(params.get("num_res_blocks", 2)),
            attention_resolutions=tuple(params.get("attention_resolutions", (4, 2, 1))),
            channel_mult=tuple(params.get("channel_mult", (1, 2, 4, 4))),
            num_heads=int(params.get("num_heads", 8)),
            context_dim=int(params.get("context_dim", 768)),
            pos_in_dim=int(gt.get("in_dim", 768)),
            pos_out_dim=int(gt.get("out_dim", 768)),
            fourier_freqs=int(gt.get("fourier_freqs", 8)),
            grounding=grounding,
            inpaint_mode=bool(params.get("inpaint_mode", False)),
        )
        kp.update(sp)
        return replace(cfg, **kp) if kp else cfg


def _spatial_family(target):
    """the key of SPATIAL_FAMILIES a grounding_tokenizer target names, or None"""
    if not target or not target.endswith(".PositionNet"):
        return None
    mod = target[:-len(".PositionNet")].rsplit(".", 1)[-1]
    return mod if mod in SPATIAL_FAMILIES else None


# A small config used by tests (CPU goldens and the GPU whole-model parity test).
# Channels are multiples of 64 (engine GEMM K-tile) and of 32 (GroupNorm32).
TINY = UNetConfig(image_size=16, model_channels=64, num_heads=4)


@dataclass(frozen=True)
class Layer:
    kind: str            # conv_in | res | st | down | up
    prefix: str          # state_dict prefix of the module
    cin: int
    cout: int
    d_head: int = 0


@dataclass
class Block:
    """One TimestepEmbedSequential (openaimodel.py:40-54)."""
    layers: List[Layer] = field(default_factory=list)
    skip_in: int = 0     # channels popped from the skip stack and concatenated (output blocks)


@dataclass
class Plan:
    cfg: UNetConfig
    input_blocks: List[Block]
    middle: Block
    output_blocks: List[Block]
    out_channels_last: int

    def all_layers(self):
        for b in self.input_blocks:
            yield from b.layers
        yield from self.middle.layers
        for b in self.output_blocks:
            yield from b.layers

    def res_layers(self) -> List[Layer]:
        return [l for l in self.all_layers() if l.kind == "res"]

    def st_layers(self) -> List[Layer]:
        return [l for l in self.all_layers() if l.kind == "st"]


def build_plan(cfg: UNetConfig) -> Plan:
    mc, heads = cfg.model_channels, cfg.num_heads
    inputs: List[Block] = [Block([Layer("conv_in", "input_blocks.0.0", cfg.in_channels, mc)])]
    chans = [mc]
    ch, ds = mc, 1
    for level, mult in enumerate(cfg.channel_mult):
        for _ in range(cfg.num_res_blocks):
            idx = len(inputs)
            layers = [Layer("res", f"input_blocks.{idx}.0", ch, mult * mc)]
            ch = mult * mc
            if ds in cfg.attention_resolutions:
                layers.append(Layer("st", f"input_blocks.{idx}.1", ch, ch, ch // heads))
            inputs.append(Block(layers))
            chans.append(ch)
        if level != len(cfg.channel_mult) - 1:
            idx = len(inputs)
            inputs.append(Block([Layer("down", f"input_blocks.{idx}.0.op", ch, ch)]))
            chans.append(ch)
            ds *= 2
    middle = Block([
        Layer("res", "middle_block.0", ch, ch),
        Layer("st", "middle_block.1", ch, ch, ch // heads),
        Layer("res", "middle_block.2", ch, ch),
    ])
    outputs: List[Block] = []
    for level, mult in list(enumerate(cfg.channel_mult))[::-1]:
        for i in range(cfg.num_res_blocks + 1):
            ich = chans.pop()
            idx = len(outputs)
            layers = [Layer("res", f"output_blocks.{idx}.0", ch + ich, mc * mult)]
            ch = mc * mult
            if ds in cfg.attention_resolutions:
                layers.append(Layer("st", f"output_blocks.{idx}.1", ch, ch, ch // heads))
            if level and i == cfg.num_res_blocks:
                layers.append(Layer("up", f"output_blocks.{idx}.{len(layers)}.conv", ch, ch))
                ds //= 2
            outputs.append(Block(layers, skip_in=ich))
    return Plan(cfg, inputs, middle, outputs, ch)


def _j(p: str, n: str) -> str:
    return n if p == "" else f"{p}.{n}"


def attn_params(p: str, C: int, kv_dim: int) -> Dict[str, Tuple[int, ...]]:
    return {
        _j(p, "to_q.weight"): (C, C),
        _j(p, "to_k.weight"): (C, kv_dim),
        _j(p, "to_v.weight"): (C, kv_dim),
        _j(p, "to_out.0.weight"): (C, C),
        _j(p, "to_out.0.bias"): (C,),
    }


def ff_params(p: str, C: int) -> Dict[str, Tuple[int, ...]]:
    return {
        _j(p, "net.0.proj.weight"): (8 * C, C),
        _j(p, "net.0.proj.bias"): (8 * C,),
        _j(p, "net.2.weight"): (C, 4 * C),
        _j(p, "net.2.bias"): (C,),
    }


def norm_params(p: str, C: int) -> Dict[str, Tuple[int, ...]]:
    return {_j(p, "weight"): (C,), _j(p, "bias"): (C,)}


def conv_params(p: str, cin: int, cout: int, k: int = 3) -> Dict[str, Tuple[int, ...]]:
    return {_j(p, "weight"): (cout, cin, k, k), _j(p, "bias"): (cout,)}


def res_params(p: str, cin: int, cout: int, te: int) -> Dict[str, Tuple[int, ...]]:
    """ResBlock (openaimodel.py:155-194)."""
    out: Dict[str, Tuple[int, ...]] = {}
    out.update(norm_params(_j(p, "in_layers.0"), cin))
    out.update(conv_params(_j(p, "in_layers.2"), cin, cout))
    out[_j(p, "emb_layers.1.weight")] = (cout, te)
    out[_j(p, "emb_layers.1.bias")] = (cout,)
    out.update(norm_params(_j(p, "out_layers.0"), cout))
    out.update(conv_params(_j(p, "out_layers.3"), cout, cout))
    if cin != cout:
        out.update(conv_params(_j(p, "skip_connection"), cin, cout, 1))
    return out


def fuser_params(p: str, C: int, ctx: int) -> Dict[str, Tuple[int, ...]]:
    """GatedSelfAttentionDense (attention.py:206-224)."""
    out: Dict[str, Tuple[int, ...]] = {_j(p, "alpha_attn"): (), _j(p, "alpha_dense"): ()}
    out[_j(p, "linear.weight")] = (C, ctx)
    out[_j(p, "linear.bias")] = (C,)
    out.update(attn_params(_j(p, "attn"), C, C))
    out.update(ff_params(_j(p, "ff"), C))
    for n in ("norm1", "norm2"):
        out.update(norm_params(_j(p, n), C))
    return out


def rela_params(p: str, C: int, ctx: int) -> Dict[str, Tuple[int, ...]]:
    """RelationCrossAttention (attention.py:284-303)."""
    out: Dict[str, Tuple[int, ...]] = {_j(p, "alpha_attn"): (), _j(p, "alpha_dense"): ()}
    out.update(attn_params(_j(p, "attn"), C, ctx))
    out.update(ff_params(_j(p, "ff"), C))
    for n in ("norm1", "norm2", "norm3"):
        out.update(norm_params(_j(p, n), C))
    return out


def block_params(t: str, C: int, ctx: int, relation: bool = True) -> Dict[str, Tuple[int, ...]]:
    """BasicTransformerBlock (attention.py:362-384), in module registration order; ``relation=False``: upstream's, without rela_fuse."""
    out: Dict[str, Tuple[int, ...]] = {}
    out.update(attn_params(_j(t, "attn1"), C, C))
    out.update(ff_params(_j(t, "ff"), C))
    out.update(attn_params(_j(t, "attn2"), C, ctx))
    for n in ("norm1", "norm2", "norm3"):
        out.update(norm_params(_j(t, n), C))
    out.update(fuser_params(_j(t, "fuser"), C, ctx))
    if relation:
        out.update(rela_params(_j(t, "rela_fuse"), C, ctx))
    return out


def st_params(p: str, C: int, ctx: int, relation: bool = True) -> Dict[str, Tuple[int, ...]]:
    """SpatialTransformer (attention.py:405-434)."""
    out: Dict[str, Tuple[int, ...]] = {}
    out.update(norm_params(_j(p, "norm"), C))
    out.update(conv_params(_j(p, "proj_in"), C, C, 1))
    out.update(block_params(_j(p, "transformer_blocks.0"), C, ctx, relation))
    out.update(conv_params(_j(p, "proj_out"), C, C, 1))
    return out


def spatial_tokenizer_params(cfg: UNetConfig) -> Dict[str, Tuple[int, ...]]:
    """position_net.* of a spatial model ({canny,hed,depth,normal}_grounding_net.py:12-35 + convnext.py), in the order of the module's state
    dict: its own two parameters, then the ConvNeXt backbone (downsample_layers, stages), then the linears"""
    dims, depths = cfg.convnext_dims, cfg.convnext_depths
    p = "position_net"
    bb = p + ".convnext_tiny_backbone"
    out: Dict[str, Tuple[int, ...]] = {}
    out[p + ".pos_embedding"] = (1, cfg.n_ground, dims[3])
    out[p + ".null_feature"] = (dims[3],)
    if cfg.ds_kind == "sem":
        out[p + ".in_conv.weight"] = (3, cfg.sem_classes, 3, 3)       # sem_grounding_net.py:22: from the one-hot classes to 3 channels
        out[p + ".in_conv.bias"] = (3,)
    out[bb + ".downsample_layers.0.0.weight"] = (dims[0], 3, 4, 4)
    out[bb + ".downsample_layers.0.0.bias"] = (dims[0],)
    out[bb + ".downsample_layers.0.1.weight"] = (dims[0],)
    out[bb + ".downsample_layers.0.1.bias"] = (dims[0],)
    for i in range(1, 4):
        out[bb + f".downsample_layers.{i}.0.weight"] = (dims[i - 1],)
        out[bb + f".downsample_layers.{i}.0.bias"] = (dims[i - 1],)
        out[bb + f".downsample_layers.{i}.1.weight"] = (dims[i], dims[i - 1], 2, 2)
        out[bb + f".downsample_layers.{i}.1.bias"] = (dims[i],)
    for i in range(4):
        C = dims[i]
        for j in range(depths[i]):
            b = bb + f".stages.{i}.{j}"
            out[b + ".gamma"] = (C,)
            out[b + ".dwconv.weight"] = (C, 1, 7, 7)
            out[b + ".dwconv.bias"] = (C,)
            out[b + ".norm.weight"] = (C,)
            out[b + ".norm.bias"] = (C,)
            out[b + ".pwconv1.weight"] = (4 * C, C)
            out[b + ".pwconv1.bias"] = (4 * C,)
            out[b + ".pwconv2.weight"] = (C, 4 * C)
            out[b + ".pwconv2.bias"] = (C,)
    out[p + ".linears.0.weight"] = (512, dims[3])
    out[p + ".linears.0.bias"] = (512,)
    out[p + ".linears.2.weight"] = (512, 512)
    out[p + ".linears.2.bias"] = (512,)
    out[p + ".linears.4.weight"] = (cfg.pos_out_dim, 512)
    out[p + ".linears.4.bias"] = (cfg.pos_out_dim,)
    return out


def param_shapes(cfg: UNetConfig) -> Dict[str, Tuple[int, ...]]:
    """state_dict name -> shape for the whole UNet, in module registration order."""
    plan = build_plan(cfg)
    te, ctx = cfg.time_embed_dim, cfg.context_dim
    out: Dict[str, Tuple[int, ...]] = {}
    out["time_embed.0.weight"] = (te, cfg.model_channels)
    out["time_embed.0.bias"] = (te,)
    out["time_embed.2.weight"] = (te, te)
    out["time_embed.2.bias"] = (te,)
    if cfg.ds_kind == "conv":
        # *_grounding_downsampler.py: Conv2d(c, 4, 4, 2, 1), SiLU, Conv2d(4, out_dim, 4, 2, 1); registered right after time_embed
        out["downsample_net.layers.0.weight"] = (4, cfg.ds_in, 4, 4)
        out["downsample_net.layers.0.bias"] = (4,)
        out["downsample_net.layers.2.weight"] = (cfg.ds_out, 4, 4, 4)
        out["downsample_net.layers.2.bias"] = (cfg.ds_out,)
    if cfg.ds_kind == "sem":
        # sem_grounding_downsampler.py:15-19: Conv2d(classes, 16, 4, 2, 1), SiLU, Conv2d(16, out_dim, 4, 2, 1)
        out["downsample_net.layers.0.weight"] = (SEM_DS_HIDDEN, cfg.sem_classes, 4, 4)
        out["downsample_net.layers.0.bias"] = (SEM_DS_HIDDEN,)
        out["downsample_net.layers.2.weight"] = (cfg.ds_out, SEM_DS_HIDDEN, 4, 4)
        out["downsample_net.layers.2.bias"] = (cfg.ds_out,)
    for l in plan.all_layers():
        if l.kind == "conv_in":
            out.update(conv_params(l.prefix, cfg.first_conv_in, l.cout))      # 9 input channels on an inpaint_mode model
        elif l.kind in ("down", "up"):
            out.update(conv_params(l.prefix, l.cin, l.cout))
        elif l.kind == "res":
            out.update(res_params(l.prefix, l.cin, l.cout, te))
        elif l.kind == "st":
            out.update(st_params(l.prefix, l.cin, ctx, cfg.relation))
        else:
            raise ValueError(l.kind)
    out.update(norm_params("out.0", plan.out_channels_last))
    out.update(conv_params("out.2", plan.out_channels_last, cfg.out_channels))
    if cfg.grounding == "text_image":
        # text_image_grounding_net.py:19-38, in module registration order
        for chain in ("linears_text", "linears_image"):
            out[f"position_net.{chain}.0.weight"] = (512, cfg.pos_in_dim + cfg.position_dim)
            out[f"position_net.{chain}.0.bias"] = (512,)
            out[f"position_net.{chain}.2.weight"] = (512, 512)
            out[f"position_net.{chain}.2.bias"] = (512,)
            out[f"position_net.{chain}.4.weight"] = (cfg.pos_out_dim, 512)
            out[f"position_net.{chain}.4.bias"] = (cfg.pos_out_dim,)
        out["position_net.null_text_feature"] = (cfg.pos_in_dim,)
        out["position_net.null_image_feature"] = (cfg.pos_in_dim,)
        out["position_net.null_position_feature"] = (cfg.position_dim,)
        return out
    if cfg.grounding == "spatial":
        out.update(spatial_tokenizer_params(cfg))
        return out
    if cfg.grounding == "keypoint":
        # keypoint_grounding_net.py:15-31, in the order of the module's state dict (its own parameters, then the linears)
        D = cfg.pos_out_dim
        out["position_net.person_embeddings"] = (cfg.max_persons, D)
        out["position_net.keypoint_embeddings"] = (KEYPOINTS, D)
        out["position_net.null_person_feature"] = (D,)
        out["position_net.null_xy_feature"] = (cfg.position_dim,)
        out["position_net.linears.0.weight"] = (512, D + cfg.position_dim)
        out["position_net.linears.0.bias"] = (512,)
        out["position_net.linears.2.weight"] = (512, 512)
        out["position_net.linears.2.bias"] = (512,)
        out["position_net.linears.4.weight"] = (D, 512)
        out["position_net.linears.4.bias"] = (D,)
        return out
    if cfg.grounding != "text":
        raise ValueError(f"grounding = {cfg.grounding!r}")
    out["position_net.null_positive_feature"] = (cfg.pos_in_dim,)
    out["position_net.null_position_feature"] = (cfg.position_dim,)
    out["position_net.linears.0.weight"] = (512, cfg.pos_in_dim + cfg.position_dim)
    out["position_net.linears.0.bias"] = (512,)
    out["position_net.linears.2.weight"] = (512, 512)
    out["position_net.linears.2.bias"] = (512,)
    out["position_net.linears.4.weight"] = (cfg.pos_out_dim, 512)
    out["position_net.linears.4.bias"] = (cfg.pos_out_dim,)
    return out


def count_params(cfg: UNetConfig) -> int:
    n = 0
    for shp in param_shapes(cfg).values():
        k = 1
        for s in shp:
            k *= s
        n += k
    return n


# --------------------------------------------------------------------------- VAE decoder
@dataclass(frozen=True)
class VAEConfig:
    """AutoencoderKL decoder hyper-parameters; defaults are GLIGEN/configs/coco2014.yaml:33-53."""
    ch: int = 128
    ch_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    z_channels: int = 4
    out_ch: int = 3
    embed_dim: int = 4
    scale_factor: float = 0.18215


VAE_TINY = VAEConfig(ch=64, ch_mult=(1, 2), num_res_blocks=1)


def vae_decoder_param_shapes(cfg: VAEConfig) -> Dict[str, Tuple[int, ...]]:
    """state_dict name -> shape of everything AutoencoderKL.decode touches (autoencoder.py:40-44,
    model.py:462-568), in the reference's naming (post_quant_conv.*, decoder.*)."""
    out: Dict[str, Tuple[int, ...]] = {}
    out.update(conv_params("post_quant_conv", cfg.embed_dim, cfg.z_channels, 1))
    nres = len(cfg.ch_mult)
    block_in = cfg.ch * cfg.ch_mult[nres - 1]
    out.update(conv_params("decoder.conv_in", cfg.z_channels, block_in))

    def resnet(p, cin, cout):
        out.update(norm_params(p + ".norm1", cin))
        out.update(conv_params(p + ".conv1", cin, cout))
        out.update(norm_params(p + ".norm2", cout))
        out.update(conv_params(p + ".conv2", cout, cout))
        if cin != cout:
            out.update(conv_params(p + ".nin_shortcut", cin, cout, 1))
    resnet("decoder.mid.block_1", block_in, block_in)
    out.update(norm_params("decoder.mid.attn_1.norm", block_in))
    for n in ("q", "k", "v", "proj_out"):
        out.update(conv_params(f"decoder.mid.attn_1.{n}", block_in, block_in, 1))
    resnet("decoder.mid.block_2", block_in, block_in)
    for lvl in reversed(range(nres)):
        block_out = cfg.ch * cfg.ch_mult[lvl]
        for i in range(cfg.num_res_blocks + 1):
            resnet(f"decoder.up.{lvl}.block.{i}", block_in, block_out)
            block_in = block_out
        if lvl != 0:
            out.update(conv_params(f"decoder.up.{lvl}.upsample.conv", block_in, block_in))
    out.update(norm_params("decoder.norm_out", block_in))
    out.update(conv_params("decoder.conv_out", block_in, cfg.out_ch))
    return out


def vae_encoder_param_shapes(cfg: VAEConfig) -> Dict[str, Tuple[int, ...]]:
    """state_dict name -> shape of everything AutoencoderKL.encode touches (autoencoder.py:34-38, Encoder model.py:368-459 with
    in_channels = out_ch, double_z and no down-level attention), in the reference's naming (encoder.*, quant_conv.*)."""
    out: Dict[str, Tuple[int, ...]] = {}
    out.update(conv_params("encoder.conv_in", cfg.out_ch, cfg.ch))
    nres = len(cfg.ch_mult)
    in_ch_mult = (1,) + tuple(cfg.ch_mult)
    block_in = cfg.ch

    def resnet(p, cin, cout):
        out.update(norm_params(p + ".norm1", cin))
        out.update(conv_params(p + ".conv1", cin, cout))
        out.update(norm_params(p + ".norm2", cout))
        out.update(conv_params(p + ".conv2", cout, cout))
        if cin != cout:
            out.update(conv_params(p + ".nin_shortcut", cin, cout, 1))
    for lvl in range(nres):
        block_in, block_out = cfg.ch * in_ch_mult[lvl], cfg.ch * cfg.ch_mult[lvl]
        for i in range(cfg.num_res_blocks):
            resnet(f"encoder.down.{lvl}.block.{i}", block_in, block_out)
            block_in = block_out
        if lvl != nres - 1:
            out.update(conv_params(f"encoder.down.{lvl}.downsample.conv", block_in, block_in))
    resnet("encoder.mid.block_1", block_in, block_in)
    out.update(norm_params("encoder.mid.attn_1.norm", block_in))
    for n in ("q", "k", "v", "proj_out"):
        out.update(conv_params(f"encoder.mid.attn_1.{n}", block_in, block_in, 1))
    resnet("encoder.mid.block_2", block_in, block_in)
    out.update(norm_params("encoder.norm_out", block_in))
    out.update(conv_params("encoder.conv_out", block_in, 2 * cfg.z_channels))
    out.update(conv_params("quant_conv", 2 * cfg.z_channels, 2 * cfg.embed_dim, 1))
    return out
