"""Rectangular (h != w) latents, host side (no GPU): the oracle against the reference's rectangular goldens
(tools/make_rect_goldens.py), the per-axis box masks, the pixel-size validation and the additive C entry points."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rect_cases as rc
import test_oracle_golden as tog
import vae_encoder_pyref
from layoutllm_t2i_amd import _lib, arch, flops, host, recipe
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, VAEConfig
from oracle import plms_ref, unet_ref, vae_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy

# the MASK_BOXES of tools/make_inpaint_goldens.py (border, sub-pixel, reversed, overlapping, empty), as stored by that tool
MASK_BOXES = np.load(os.path.join(GOLD, "inpaint_masks.npz"))["boxes"]


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def run_oracle(case):
    k, nm = case["kind"], case["name"]
    inp = {a: T(v) for a, v in rc.case_inputs(case).items()}
    tag = f"golden.{nm}"
    if k == "rela":
        sd = {"r." + n: v for n, v in tog.sd_for(tag, arch.rela_params("", case["C"], rc.CTX)).items()}
        return unet_ref.relation_cross_attention(sd, "r", inp["x"], inp["relations"], inp["boxes"], inp["masks"], case["h"], case["w"], case["heads"])
    if k == "spatial_transformer":
        sd = {"s." + n: v for n, v in tog.sd_for(tag, arch.st_params("", case["C"], rc.CTX)).items()}
        return unet_ref.spatial_transformer(sd, "s", inp["x"], inp["context"], inp["objs"], inp["relations"], inp["boxes"], inp["masks"],
                                            case["heads"], case["scale"])
    if k == "down":
        sd = tog.sd_for(tag, arch.conv_params("op", case["C"], case["C"]))
        return torch.nn.functional.conv2d(inp["x"], sd["op.weight"], sd["op.bias"], stride=2, padding=1)
    if k == "up":
        sd = tog.sd_for(tag, arch.conv_params("conv", case["C"], case["C"]))
        y = torch.nn.functional.interpolate(inp["x"], scale_factor=2, mode="nearest")
        return torch.nn.functional.conv2d(y, sd["conv.weight"], sd["conv.bias"], padding=1)
    if k == "unet":
        fc = {a: T(v) for a, v in recipe.sd_first_conv(TINY, 0).items()} if case["sdconv"] else None
        return unet_ref.unet_forward(tog.tiny_sd(), TINY, inp["x"], torch.tensor(case["t"]), inp["context"], inp["relations"], inp["boxes"],
                                     inp["masks"], inp["positive_embeddings"], fuser_scale=case["scale"], first_conv=fc)
    if k == "vae":
        sd = {n: T(np.asarray(v)) for n, v in recipe.vae_state_dict(VAE_TINY, 0).items()}
        return vae_ref.decode(sd, inp["z"], VAE_TINY.ch_mult, VAE_TINY.num_res_blocks, VAE_TINY.scale_factor)
    raise ValueError(k)


MODULE_CASES = [c for c in rc.CASES if c["kind"] in ("rela", "spatial_transformer", "down", "up", "unet", "vae")]


@pytest.mark.parametrize("case", MODULE_CASES, ids=[c["name"] for c in MODULE_CASES])
def test_oracle_matches_rect_reference(case):
    """test_oracle_golden.test_oracle_matches_reference's comparison and tolerances, on the h != w goldens."""
    with torch.no_grad():
        out = run_oracle(case).numpy()
    ref = gold(case["name"])["out"]
    assert out.shape == ref.shape and np.isfinite(ref).all()
    if case["kind"] in ("spatial_transformer", "unet", "down"):
        exp = {"spatial_transformer": (case["h"], case["w"]), "unet": (case["h"], case["w"]), "down": (case["h"] // 2, case["w"] // 2)}[case["kind"]]
        assert ref.shape[-2:] == exp
    scale = max(1.0, float(np.nanmax(np.abs(ref))))
    tog.close(out, ref, rtol=1e-4, atol=3e-5 * scale)


def test_rect_boxes_exercise_clamp_break_and_orientation():
    """The rela / transformer box set: the rectangles at 8 x 12 and 12 x 8 differ, box 1 clamps, sample 0 breaks at box 2."""
    boxes, masks = rc.rect_boxes(2)
    rw, nw, pw = host.box_rects(boxes, masks, 8, 12)
    rt, nt, pt = host.box_rects(boxes, masks, 12, 8)
    assert list(nw) == [2, 4] and list(nt) == [2, 4] and not pw.any() and not pt.any()
    assert not np.array_equal(rw, rt)
    assert rw[0, 1, 3] == 12 and rt[0, 1, 3] == 8 and boxes[0, 1, 2] * 12 > 12          # right edge clamped to w
    assert (rw[0, 2:] == 0).all()                                                       # the valid-looking box 3 is dropped with box 2
    # swapping h and w on the wide golden's inputs changes the result: the two orientations test different rectangles
    a, b = gold("rela_rect_wide")["out"], gold("rela_rect_tall")["out"]
    assert a.shape == b.shape == (2, 96, 64) and not np.allclose(a, b)


def test_fp32_encoder_mirror_matches_rect_reference_golden():
    g = gold("vae_enc_tiny_rect")
    cfg = VAE_TINY
    assert g["x"].shape == (2, 3, 32, 48) and g["z"].shape == (2, 4, 16, 24)
    sd = {k: T(np.asarray(v)) for k, v in {**recipe.vae_state_dict(cfg, 0), **recipe.vae_encoder_state_dict(cfg, 0)}.items()}
    with torch.no_grad():
        z, mean = vae_encoder_pyref.encode(sd, T(g["x"]), cfg.ch_mult, cfg.num_res_blocks, T(g["noise"]), cfg.scale_factor)
    for got, name in ((mean, "mean"), (z, "z")):
        ref = T(g[name])
        r = float((got - ref).norm() / ref.norm())
        assert got.shape == ref.shape and r < 1e-6, (name, r)
    torch.manual_seed(int(g["seed"]))
    assert torch.equal(torch.randn(tuple(mean.shape)), T(g["noise"]))


def test_plms_rect_tiny_matches_reference():
    case = rc.case("plms_rect_tiny")
    inp = {a: T(v) for a, v in rc.case_inputs(case).items()}
    with torch.no_grad():
        out = plms_ref.plms_sample(tog.make_eps_fn(case, inp, tog.tiny_sd(), TINY), inp["x"], case["S"], case["alpha_type"])
    ref = gold("plms_rect_tiny")["out"]
    assert ref.shape == (2, 4, 16, 24)
    err = np.abs(out.numpy() - ref).max() / np.abs(ref).max()
    assert err < 2e-4, err


def test_plms_inpaint_rect_golden_holds_the_rule_mask():
    """The mask the reference sampler was given is the per-axis rectangle rule, and equals host.draw_masks_from_boxes((H, W))."""
    case = rc.case("plms_inpaint_rect_tiny")
    inp = rc.case_inputs(case)
    g = gold("plms_inpaint_rect_tiny")
    assert g["out"].shape == (2, 4, 16, 24) and g["x0"].shape == (1, 4, 16, 24) and g["mask"].shape == (2, 1, 16, 24)
    assert np.array_equal(g["mask"], rc.rect_mask_rule(inp["boxes"], 16, 24))
    assert np.array_equal(host.draw_masks_from_boxes(inp["boxes"], (16, 24)).numpy(), g["mask"])
    assert 0 < g["mask"].mean() < 1
    assert g["draw_shapes"].tolist()[0] == [1, 4, 16, 24]


# ------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("size", [(8, 12), (13, 16), (64, 96)])
def test_rect_masks_equal_the_rule(size):
    H, W = size
    got = host.draw_masks_from_boxes(T(MASK_BOXES), size)
    assert got.dtype == torch.float32 and tuple(got.shape) == (MASK_BOXES.shape[0], 1, H, W)
    want = rc.rect_mask_rule(MASK_BOXES, H, W)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(host.draw_masks_from_boxes(MASK_BOXES, [H, W]).numpy(), want)             # numpy boxes, list size
    # the orientation matters for these boxes
    assert not np.array_equal(host.draw_masks_from_boxes(MASK_BOXES, (W, H)).numpy().transpose(0, 1, 3, 2), want)


@pytest.mark.parametrize("size", [64, 16, 13])
def test_int_and_square_tuple_sizes_reproduce_the_reference_masks(size):
    g = gold("inpaint_masks")
    assert np.array_equal(host.draw_masks_from_boxes(T(g["boxes"]), size).numpy(), g[f"mask_{size}"])
    assert np.array_equal(host.draw_masks_from_boxes(T(g["boxes"]), (size, size)).numpy(), g[f"mask_{size}"])
    assert np.array_equal(rc.rect_mask_rule(g["boxes"], size, size), g[f"mask_{size}"])             # the rule itself, vs the reference


# ------------------------------------------------------------------------------------------- interface
class _Auto:
    def __init__(self, cfg):
        self.cfg = cfg


def test_height_width_validation():
    assert itf.latent_hw() == (64, 64)
    assert itf.latent_hw(512, 768) == (64, 96) and itf.latent_hw(768, 512) == (96, 64)
    assert itf.latent_hw(32, 48, _Auto(VAE_TINY)) == (16, 24)                   # vae_factor 2: multiples of 16 pixels
    for bad in ((500, 512), (512, 520), (0, 512), (512, -64), (512.0, 512), (True, 512), (40, 48, _Auto(VAE_TINY))):
        with pytest.raises(ValueError):
            itf.latent_hw(*bad)
    # the entries validate before they touch a model, a tokenizer or the GPU
    none5 = (None, None, None, None, None)
    with pytest.raises(ValueError, match="height"):
        itf.generate_one_image_sized(none5, "a cat", ["cat"], [[0.1, 0.1, 0.3, 0.3]], height=500, width=512)
    with pytest.raises(ValueError, match="width"):
        itf.generate_batch_images_sized(none5, ["a cat"], [["cat"]], [[[0.1, 0.1, 0.4, 0.4]]], height=512, width=100)
    with pytest.raises(ValueError, match="width"):
        itf.generate_batch_images_sharded(none5, ["a cat"], [["cat"]], [[[0.1, 0.1, 0.4, 0.4]]], width=72)
    import inspect
    for f in (itf.generate_one_image_sized, itf.generate_batch_images_sized):
        p = inspect.signature(f).parameters
        assert p["height"].default is None and p["width"].default is None          # None = the reference's 64 x 64 latent (512 pixels)
    assert itf.latent_hw(None, 768) == (64, 96) and itf.latent_hw(None, None, _Auto(VAE_TINY)) == (64, 64)
    assert list(inspect.signature(itf.generate_one_image_sized).parameters)[:7] == list(inspect.signature(itf.generate_one_image).parameters)
    assert list(inspect.signature(itf.generate_batch_images_sized).parameters)[:7] == list(inspect.signature(itf.generate_batch_images).parameters)


def test_prompt_noise_and_synth_inputs_take_hw():
    a = itf.prompt_noise([3, 4], (16, 24))
    assert tuple(a.shape) == (2, 4, 16, 24) and torch.equal(a[1:], itf.prompt_noise([4], (16, 24)))
    assert torch.equal(itf.prompt_noise([3], 16), itf.prompt_noise([3], (16, 16)))
    d = recipe.synth_inputs(TINY, 2, (16, 24), n_boxes=4)
    assert d["x"].shape == (2, 4, 16, 24)
    sq, sq2 = recipe.synth_inputs(TINY, 2, 16, n_boxes=4), recipe.synth_inputs(TINY, 2, (16, 16), n_boxes=4)
    assert all(np.array_equal(sq[k], sq2[k]) for k in sq)


def test_load_input_image_resizes_to_w_h():
    from PIL import Image
    im = Image.fromarray((np.clip(recipe.uniform("rect.img", (40, 56, 3), 4), 0, 1) * 255).astype(np.uint8))
    x = itf.load_input_image(im, (32, 48))
    assert tuple(x.shape) == (1, 3, 32, 48)
    ref = torch.from_numpy(np.array(im.convert("RGB").resize((48, 32)), dtype=np.uint8)).permute(2, 0, 1)
    assert torch.equal(x, (ref.float().unsqueeze(0) / 255 - 0.5) / 0.5)
    assert torch.equal(itf.load_input_image(im, 32), itf.load_input_image(im, (32, 32)))


def test_flops_take_hw():
    cfg = arch.UNetConfig()
    sq = flops.unet_forward_flops(cfg, 64)
    assert flops.unet_forward_flops(cfg, (64, 64)) == sq
    wide, tall = flops.unet_forward_flops(cfg, (64, 96)), flops.unet_forward_flops(cfg, (96, 64))
    assert wide == tall and sq < wide < flops.unet_forward_flops(cfg, 80) < flops.unet_forward_flops(cfg, 96)
    v = VAEConfig()
    assert flops.vae_encoder_flops(v, 1, (512, 512)) == flops.vae_encoder_flops(v, 1, 512)
    assert flops.vae_encoder_flops(v, 1, 512) < flops.vae_encoder_flops(v, 1, (512, 768)) < flops.vae_encoder_flops(v, 1, 768)


# ------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_are_exported_under_abi_15():
    l = _lib.lib()
    assert l.gl_abi_version() == 15 and _lib.ABI_VERSION == 15
    for name in ("gl_set_conditioning_hw", "gl_vae_decode_hw", "gl_vae_encode_hw"):
        assert name in _lib.PROTOTYPES and getattr(l, name) is not None
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gligen_hip.h")).read()
    for name in ("gl_set_conditioning_hw(", "gl_vae_decode_hw(", "gl_vae_encode_hw(", "9216 tokens"):
        assert name in hdr, name


def test_hw_entries_reject_bad_arguments_on_the_host():
    """No GPU is touched: the handle checks come first (GL_ERR_BAD_ARG = -1)."""
    l = _lib.lib()
    assert l.gl_set_conditioning_hw(None, None, None, None, None, None, 1, 77, 10, 16, 24, None) == -1
    assert l.gl_vae_decode_hw(None, None, 1, 8, 12, None, 0, None) == -1
    assert l.gl_vae_encode_hw(None, None, 1, 32, 48, None, None, 0, None) == -1
    h = _lib.create_vae(VAE_TINY, encoder=True)
    try:        # a handle without weights, any shape: refused before a launch
        assert l.gl_vae_encode_hw(h, None, 1, 32, 48, None, None, 0, None) == -1
    finally:
        l.gl_vae_destroy(h)
