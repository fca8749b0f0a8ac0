"""CPU tests (no GPU) of the inpaint_mode UNet (GLIGEN's checkpoint_inpainting_text*.pth, a 9-channel first conv): config parsing, the
packed first conv, the engine's weight table, the host-side refusals of the new ABI entry, the interface's extra builder and error paths,
and tests/inpaint9_ref.py against the reference's own outputs (tests/golden/ip9_*.npz)."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import inpaint9_cases as ic
import inpaint9_ref
import ti_ref
from layoutllm_t2i_amd import _lib, arch, flops, host, recipe, weights
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY, UNetConfig
from layoutllm_t2i_amd.model import UNetModel

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
TI_TARGET = "ldm.modules.diffusionmodules.text_image_grounding_net.PositionNet"


def _ensure_built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)


# ------------------------------------------------------------------------------------------- configuration
def test_from_dict_reads_inpaint_mode():
    base = dict(model_channels=64, num_heads=4)
    ip = UNetConfig.from_dict({**base, "inpaint_mode": True}, allow_inpaint=True)
    assert ip.inpaint_mode is True and ip.first_conv_in == 9 and ip.in_channels == 4 and ip.out_channels == 4
    assert dataclasses.replace(ip, image_size=16) == ic.IP_TINY
    with pytest.raises(NotImplementedError, match="allow_inpaint=True"):       # a caller that does not say it feeds the extra is still refused
        UNetConfig.from_dict({**base, "inpaint_mode": True})
    tx = UNetConfig.from_dict({**base, "inpaint_mode": False})
    assert tx.inpaint_mode is False and tx.first_conv_in == 4 and UNetConfig.from_dict(base) == tx and UNetConfig().first_conv_in == 4
    ti = UNetConfig.from_dict({**base, "inpaint_mode": True, "grounding_tokenizer": {"target": TI_TARGET, "params": {}}}, allow_inpaint=True)
    assert dataclasses.replace(ti, image_size=16) == ic.IP_TI_TINY
    # GLIGEN's published layout: [320, 9, 3, 3]
    assert arch.param_shapes(UNetConfig(inpaint_mode=True))["input_blocks.0.0.weight"] == (320, 9, 3, 3)
    for mode in (True, False):          # the reference stops at a breakpoint() for the combination (openaimodel.py:437-438)
        with pytest.raises(NotImplementedError, match="grounding_downsampler"):
            UNetConfig.from_dict({**base, "inpaint_mode": mode, "grounding_downsampler": {"target": "x"}}, allow_inpaint=True)


def test_param_shapes_differ_in_the_first_conv_only():
    for a, b in ((TINY, ic.IP_TINY), (dataclasses.replace(TINY, grounding="text_image"), ic.IP_TI_TINY)):
        sa, sb = arch.param_shapes(a), arch.param_shapes(b)
        assert list(sa) == list(sb)
        assert {k for k in sa if sa[k] != sb[k]} == {"input_blocks.0.0.weight"} and sb["input_blocks.0.0.weight"] == (64, 9, 3, 3)
    assert arch.build_plan(ic.IP_TINY).input_blocks[0].layers[0].cin == 4            # the plan keeps the latent's channel count


def test_flops_count_the_five_extra_channels():
    for hw, n in ((16, 256), ((8, 16), 128)):
        d = flops.unet_forward_flops(ic.IP_TINY, hw) - flops.unet_forward_flops(TINY, hw)
        assert d == 2.0 * n * 9 * 5 * 64
    assert flops.unet_forward_flops(UNetConfig(), 64) == pytest.approx(1.1477e12, rel=1e-3)      # the text figure is unchanged


# ------------------------------------------------------------------------------------------- weights
def test_packed_first_conv_is_hi_hi_lo_by_hand():
    w = T(recipe.state_dict(ic.IP_TINY, 0, only_prefix="input_blocks.0.0.")["input_blocks.0.0.weight"])
    assert tuple(w.shape) == (64, 9, 3, 3)
    hi = w.half().float()
    lo = (w - hi).half().float()
    assert float(lo.abs().max()) > 0                                                  # recipe weights are not fp16-representable
    want = weights.pack_conv3x3(torch.cat([hi, hi, lo], dim=1), 64)
    got = weights.pack_first_conv(w, weights.CIN_PAD)
    assert got.dtype == torch.float16 and tuple(got.shape) == (64, 9 * 64) and torch.equal(got, want)
    # by hand: K = (tap, channel) inside the one 64-channel block; channels [0, 9) Whi, [9, 18) Whi, [18, 27) Wlo, [27, 64) zero
    g = got.view(64, 3, 3, 64)
    for part, src in ((0, hi), (1, hi), (2, lo)):
        assert torch.equal(g[..., 9 * part:9 * part + 9].float(), src.permute(0, 2, 3, 1))
    assert float(g[..., 27:].abs().max()) == 0.0


@pytest.mark.parametrize("split", [False, True], ids=["compact", "split"])
def test_weight_table_of_an_inpaint_handle(split):
    """same names, offsets' order and packed shapes as the text table, minus sd_first_conv.*; the packer fills it from a [mc, 9, 3, 3] tensor"""
    _ensure_built()
    cfg = dataclasses.replace(ic.IP_TINY, split_weights=split)
    h, ht = _lib.create_engine(cfg), _lib.create_engine(dataclasses.replace(TINY, split_weights=split))
    try:
        table, total = _lib.weight_table(h)
        text_table, text_total = _lib.weight_table(ht)
    finally:
        _lib.lib().gl_destroy(h)
        _lib.lib().gl_destroy(ht)
    sd_rows = [t for t in text_table if t[0].startswith("sd_first_conv.")]
    assert [t[0] for t in sd_rows] == ["sd_first_conv.w", "sd_first_conv.b"]
    strip = lambda tab: [(n, nb, dt, shp) for n, off, nb, dt, shp in tab if not n.startswith("sd_first_conv.")]
    assert strip(table) == strip(text_table) and len(table) == len(text_table) - 2
    assert dict((t[0], t[4]) for t in table)["input_blocks.0.0.w"] == (64, 9 * 64)
    pad = lambda nb: (nb + 255) // 256 * 256
    assert total == text_total - sum(pad(t[2]) for t in sd_rows)
    # offsets before the removed slots are those of the text table
    first_sd = text_table.index(sd_rows[0])
    assert table[:first_sd] == text_table[:first_sd]
    sd = recipe.state_dict(cfg, 0)
    P = weights.pack_state_dict(sd, cfg, "cpu")
    assert P.flat.numel() == total and set(P.w) == {t[0] for t in table} and P.has_sd_conv is False
    assert torch.equal(P.w["input_blocks.0.0.w"], weights.pack_first_conv(T(sd["input_blocks.0.0.weight"]), 64))
    # the shape check knows the 9-channel tensor: a text state dict does not load into an inpaint config, nor the other way round
    with pytest.raises(ValueError, match=r"input_blocks.0.0.weight: shape \(64, 4, 3, 3\) != expected \(64, 9, 3, 3\)"):
        weights.pack_state_dict(recipe.state_dict(TINY, 0), cfg, "cpu")
    with pytest.raises(ValueError, match=r"input_blocks.0.0.weight: shape \(64, 9, 3, 3\)"):
        weights.pack_state_dict(sd, dataclasses.replace(TINY, split_weights=split), "cpu")
    with pytest.raises(ValueError, match="no SD first conv"):
        weights.pack_state_dict(sd, cfg, "cpu", sd_first_conv=recipe.sd_first_conv(TINY, 0))


def test_config_struct_and_create_limits():
    _ensure_built()
    l = _lib.lib()
    assert ctypes.sizeof(_lib.UNetConfigC) == l.gl_sizeof_unet_config() and l.gl_abi_version() == 15
    assert _lib.unet_config_c(TINY).inpaint_mode == 0 and _lib.unet_config_c(ic.IP_TINY).inpaint_mode == 1
    for cfg, ok in ((dataclasses.replace(ic.IP_TINY, in_channels=31, out_channels=31), True),       # 2 * 31 + 1 = 63 <= 64
                    (dataclasses.replace(ic.IP_TINY, in_channels=32, out_channels=32), False),
                    (dataclasses.replace(TINY, in_channels=64, out_channels=64), True)):
        cc, h = _lib.unet_config_c(cfg), ctypes.c_void_p()
        rc = l.gl_create(ctypes.byref(cc), ctypes.byref(h))
        assert (rc == 0) == ok, (cfg.in_channels, cfg.inpaint_mode, rc)
        if rc == 0:
            l.gl_destroy(h)
    cc, h = _lib.unet_config_c(ic.IP_TINY), ctypes.c_void_p()
    cc.inpaint_mode = 2
    assert l.gl_create(ctypes.byref(cc), ctypes.byref(h)) != 0


def test_abi_entry_refuses_on_the_host_side():
    """gl_set_inpaint_extra on a handle without inpaint_mode, and before any conditioning call, returns GL_ERR_BAD_ARG (-1) with a message
    before it reads an argument; gl_pack_latent_extra checks its shapes: no GPU, nothing launched"""
    _ensure_built()
    l = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    htx, hip = _lib.create_engine(TINY), _lib.create_engine(ic.IP_TINY)
    try:
        assert l.gl_set_inpaint_extra(htx, p, 1, None) == -1
        assert _lib.last_error(htx).startswith("gl_set_inpaint_extra:") and "inpaint_mode = 0" in _lib.last_error(htx)
        assert l.gl_set_inpaint_extra(hip, p, 1, None) == -1
        assert "no conditioning call" in _lib.last_error(hip)
        assert l.gl_set_inpaint_extra(None, p, 1, None) == -1
        assert l.gl_unet_forward(hip, p, None, 1.0, 1, 1.0, 0, p, 0, None) == -1             # not conditioned
    finally:
        l.gl_destroy(htx)
        l.gl_destroy(hip)
    for B, Bs, C, Ce, hw, Cpad, reps, split in ((2, 3, 4, 5, 16, 64, 1, 1), (2, 1, 4, 5, 16, 26, 1, 1), (2, 1, 4, 5, 16, 8, 1, 0), (2, 1, 4, 0, 16, 64, 1, 0),
                                                (0, 1, 4, 5, 16, 64, 1, 0), (2, 1, 4, 5, 16, 64, 0, 0)):
        assert l.gl_pack_latent_extra(p, p, B, Bs, C, Ce, hw, Cpad, reps, split, p, None) == -1
    assert l.gl_pack_latent_extra(None, p, 1, 1, 4, 5, 1, 64, 1, 0, p, None) == -1 and l.gl_pack_latent_extra(p, None, 1, 1, 4, 5, 1, 64, 1, 0, p, None) == -1


# ------------------------------------------------------------------------------------------- tests/inpaint9_ref.py vs the reference
_SD = {}


def sd_of(cfg):
    if cfg not in _SD:
        _SD[cfg] = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    return _SD[cfg]


def grounding_of(cfg, inp):
    keys = ti_ref.KEYS if cfg.grounding == "text_image" else ("boxes", "masks", "positive_embeddings")
    return {k: inp[k] for k in keys}


@pytest.mark.parametrize("case", ic.UNET_CASES, ids=[c["name"] for c in ic.UNET_CASES])
def test_inpaint9_ref_matches_reference(case):
    """the tolerance of tests/test_oracle_golden.py::test_oracle_matches_reference, which pins unet_tiny_*"""
    cfg = ic.cfg_of(case)
    inp = {a: T(v) for a, v in ic.case_inputs(case).items()}
    g = grounding_of(cfg, inp)
    null = case["grounding"] == "null"
    with torch.no_grad():
        out = inpaint9_ref.unet_forward(sd_of(cfg), cfg, inp["x"], inp["extra"], torch.tensor(case["t"]), inp["uc"] if null else inp["context"],
                                        inp["relations"], inpaint9_ref.null_grounding(g) if null else g, fuser_scale=case["scale"])
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    assert out.shape == ref.shape
    scale = max(1.0, float(np.nanmax(np.abs(ref))))
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-4, atol=3e-5 * scale, equal_nan=True)


def test_goldens_see_the_extra():
    """the fixtures can tell: the mirror with the extra zeroed, or with its mask channel inverted, is far from the reference's output"""
    case = ic.by_name("ip9_unet_tiny_s1")
    inp = {a: T(v) for a, v in ic.case_inputs(case).items()}
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    flipped = inp["extra"].clone()
    flipped[:, 4] = 1 - flipped[:, 4]
    for extra in (torch.zeros_like(inp["extra"]), flipped):
        with torch.no_grad():
            out = inpaint9_ref.unet_forward(sd_of(ic.IP_TINY), ic.IP_TINY, inp["x"], extra, torch.tensor(case["t"]), inp["context"], inp["relations"],
                                            grounding_of(ic.IP_TINY, inp)).numpy()
        assert np.linalg.norm(out - ref) / np.linalg.norm(ref) > 1e-2
    # extra values are not fp16-representable, the mask channel is 0 / 1 with both present
    e = inp["extra"]
    assert float((e[:, :4] - e[:, :4].half().float()).abs().max()) > 0 and set(e[:, 4].unique().tolist()) == {0.0, 1.0}


# ------------------------------------------------------------------------------------------- interface
def test_extra_builder_is_bitwise_the_reference_extra():
    case = ic.by_name("ip9_extra")
    inp = ic.case_inputs(case)
    mask = host.draw_masks_from_boxes(inp["boxes"], case["hw"])
    ref = np.load(os.path.join(GOLD, "ip9_extra.npz"))["out"]
    out = itf.build_inpainting_extra(T(inp["z0"]), mask)
    assert out.dtype == torch.float32 and tuple(out.shape) == (5, 5, 16, 16) == ref.shape
    assert np.array_equal(out.numpy(), ref)
    assert np.array_equal(ic.make_extra(inp["z0"], mask.numpy()), ref)                 # the case table's own builder
    # a per-sample z0 works the same way
    z5 = T(inp["z0"]).repeat(5, 1, 1, 1)
    assert torch.equal(itf.build_inpainting_extra(z5, mask), out)


class _M:
    def __init__(self, cfg):
        self.cfg = cfg


def _bare_model(cfg):
    return UNetModel.from_packed(None, cfg, "cpu")


def test_missing_extra_names_the_key():
    m = _bare_model(ic.IP_TINY)
    for d in ({}, {"inpainting_extra_input": None}):
        with pytest.raises(ValueError, match="inpainting_extra_input"):
            m.inpaint_extra_of(d)
    e = torch.zeros(1, 5, 16, 16)
    assert m.inpaint_extra_of({"inpainting_extra_input": e}) is e
    # every other model ignores the key, as the reference does
    assert _bare_model(TINY).inpaint_extra_of({"inpainting_extra_input": e}) is None and _bare_model(TINY).inpaint_extra_of({}) is None


def test_restore_first_conv_on_an_inpaint_model_switches_nothing(capsys):
    m = _bare_model(ic.IP_TINY)
    m.restore_first_conv_from_SD()
    m.restore_first_conv_from_SD()
    assert m.first_conv_type == "GLIGEN" and m.use_sd_conv is False
    assert capsys.readouterr().out.count("not restorable") == 1
    with pytest.raises(RuntimeError, match="SD first-conv weights"):                   # the text model's behaviour is unchanged
        _bare_model(TINY).restore_first_conv_from_SD()


def test_inpaint_model_without_input_image_raises_before_anything_runs():
    am = (_M(ic.IP_TINY), None, None, None, {})
    with pytest.raises(ValueError, match="input_image"):
        itf.run_one_image(am, dict(batch_size=1), dict(prompt="x", phrases=["a"], locations=[[0, 0, 1, 1]]), None)
    with pytest.raises(ValueError, match="input_image"):
        itf.run_batch_images(am, dict(batch_size=1), dict(prompts=["x"], phrases=[["a"]], locations=[[[0, 0, 1, 1]]], input_image=None), None)
    assert am[4] == {}                                                                 # refused before the config was touched


def test_sharded_load_refuses_an_inpaint_checkpoint(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda: 0)
    monkeypatch.setattr(itf, "load_all_models", lambda ckpt, device, strict=None: (_M(ic.IP_TINY), None, None, None, {}))
    with pytest.raises(NotImplementedError, match="inpaint_mode checkpoint"):
        itf.load_all_models_sharded("x.pth", "cpu")
