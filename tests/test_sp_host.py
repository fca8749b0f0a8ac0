"""CPU tests (no GPU) of the spatial grounding families (GLIGEN's canny / hed / depth / normal checkpoints): config parsing and its refusals,
parameter names against the reference's, gl_create and the weight table, the family check of the conditioning entries, the ABI, the gamma fold,
the nearest / bicubic tables against torch, prepare_batch_spatial against the reference's own batch, the interface's refusals, and
tests/sp_ref.py against the reference's own outputs (tests/golden/sp_*.npz)."""
import ctypes
import dataclasses
import hashlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import sp_cases as sc
import sp_ref
from layoutllm_t2i_amd import _lib, arch, recipe, spatial, weights
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY, UNetConfig
from layoutllm_t2i_amd.model import GroundingNetInput, SpatialGroundingNetInput, UNetModel, grounding_input_for

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
FAMS = ("canny", "hed", "depth", "normal")


def _ensure_built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)


def _params(family="canny", tok=None, ds=None, **kw):
    t, d = sc.targets(family)
    dsp = {"out_dim": 1} if family == "hed" else {"resize_input": 256, "out_dim": 8}
    return {"model_channels": 64, "num_heads": 4, **kw,
            "grounding_tokenizer": {"target": tok or t, "params": {"resize_input": 256, "out_dim": 768}},
            "grounding_downsampler": {"target": ds or d, "params": dsp}}


# ------------------------------------------------------------------------------------------- configuration
@pytest.mark.parametrize("family", FAMS)
def test_from_dict_accepts_the_four_pairs(family):
    cfg = UNetConfig.from_dict(_params(family), allow_spatial=True)
    _, kind, cin, cout = arch.SPATIAL_FAMILIES[family + "_grounding_net"]
    assert cfg.grounding == "spatial" and cfg.relation is False and (cfg.ds_kind, cfg.ds_in, cfg.ds_out) == (kind, cin, cout)
    assert cfg.n_ground == 64 == cfg.max_objs and cfg.sp_resize_input == 256 and cfg.ds_resize_input == 256
    assert cfg.first_conv_in == 4 + cout == {"canny": 12, "hed": 5, "depth": 12, "normal": 12}[family]
    assert cfg.ds_latent == 64 and cfg.convnext_depths == (3, 3, 9, 3) and cfg.convnext_dims == (96, 192, 384, 768)
    assert _lib.unet_config_c(cfg).grounding == 4 and _lib.unet_config_c(cfg).max_objs == 64


def test_from_dict_refusals_name_the_downsampler():
    sem_t, sem_d = sc.targets("sem")
    bad = [
        (_params(), {}),                                                                    # a downsampler without the flag
        (_params(), dict(allow_inpaint=True, allow_keypoint=True)),
        (_params(ds="x"), dict(allow_spatial=True)),                                        # any other downsampler target
        (_params(tok=sem_t, ds=sem_d), dict(allow_spatial=True)),                           # the sem targets
        (_params(ds=sem_d), dict(allow_spatial=True)),
        (_params(inpaint_mode=True), dict(allow_spatial=True, allow_inpaint=True)),         # with inpaint_mode
        (_params(inpaint_mode=True), dict(allow_spatial=True)),
        (_params("canny", ds=sc.targets("hed")[1]), dict(allow_spatial=True)),              # tokenizer / downsampler mismatch
        (_params("hed", ds=sc.targets("depth")[1]), dict(allow_spatial=True)),
        ({"grounding_downsampler": {"target": sc.targets("canny")[1]}}, dict(allow_spatial=True)),      # on a text tokenizer
        ({"grounding_downsampler": {"target": "x"}}, {}),
    ]
    for params, kw in bad:
        with pytest.raises(NotImplementedError, match="grounding_downsampler"):
            UNetConfig.from_dict(params, **kw)
    no_ds = {k: v for k, v in _params().items() if k != "grounding_downsampler"}
    with pytest.raises(NotImplementedError, match="grounding_downsampler"):                # the tokenizer without its downsampler
        UNetConfig.from_dict(no_ds, allow_spatial=True)
    with pytest.raises(ValueError, match="resize_input"):                                   # 196 tokens: over the fuser's 64
        p = _params()
        p["grounding_tokenizer"]["params"]["resize_input"] = 448
        UNetConfig.from_dict(p, allow_spatial=True)


def test_defaults_are_unchanged():
    base = {"model_channels": 64, "num_heads": 4}
    cfg = UNetConfig.from_dict(base)
    assert cfg == UNetConfig.from_dict(base, allow_spatial=True) == dataclasses.replace(TINY, image_size=64)
    assert (cfg.ds_kind, cfg.ds_out, cfg.first_conv_in, cfg.n_ground) == ("", 0, 4, 30)
    assert _lib.UNetConfigC._fields_[-1][0] == "no_relation"          # the struct is the parent commit's: the extra channels go in by an entry


def test_param_shapes_differ_from_the_text_model_in_three_places():
    z = np.load(os.path.join(GOLD, "sp_params.npz"))
    want = {str(n): tuple(int(v) for v in str(s).split(",")) if str(s) else () for n, s in zip(z["names"], z["shapes"])}
    got = arch.param_shapes(sc.CANNY_TINY)
    assert got == want and list(got) == [str(n) for n in z["names"]]          # names, shapes and the state dict's order
    text = arch.param_shapes(dataclasses.replace(TINY, relation=False))
    body = lambda d: {k: v for k, v in d.items() if not k.startswith(("position_net.", "downsample_net.")) and k != "input_blocks.0.0.weight"}
    assert body(got) == body(text)
    assert got["input_blocks.0.0.weight"] == (64, 12, 3, 3) and text["input_blocks.0.0.weight"] == (64, 4, 3, 3)
    assert arch.param_shapes(sc.HED_TINY)["input_blocks.0.0.weight"] == (64, 5, 3, 3)
    assert arch.param_shapes(sc.sp_cfg(TINY, "normal", 64))["input_blocks.0.0.weight"] == (64, 12, 3, 3)
    assert arch.param_shapes(sc.sp_cfg(TINY, "normal", 64))["downsample_net.layers.0.weight"] == (4, 3, 4, 4)
    assert not any(k.startswith("downsample_net.") for k in arch.param_shapes(sc.HED_TINY))
    assert not any(".rela_fuse." in k for k in got)


# ------------------------------------------------------------------------------------------- gl_create, the table, the entries
def _create_rc(cfg, extra=None, **fields):
    """gl_create's code, or with ``extra`` that of gl_set_extra_channels(extra) on the created handle"""
    l = _lib.lib()
    cc, h = _lib.unet_config_c(cfg), ctypes.c_void_p()
    for k, v in fields.items():
        setattr(cc, k, v)
    rc = l.gl_create(ctypes.byref(cc), ctypes.byref(h))
    if rc == 0:
        if extra is not None:
            rc = l.gl_set_extra_channels(h, extra)
        l.gl_destroy(h)
    return rc


def test_gl_create():
    _ensure_built()
    assert _create_rc(sc.CANNY_TINY) == 0 and _create_rc(sc.HED_TINY) == 0
    assert _create_rc(sc.CANNY_TINY, extra=8) == 0 and _create_rc(sc.CANNY_TINY, extra=1) == 0 and _create_rc(sc.CANNY_TINY, extra=0) == 0
    assert _create_rc(sc.CANNY_TINY, no_relation=0) == -2
    assert _create_rc(sc.CANNY_TINY, inpaint_mode=1) == -2
    assert _create_rc(sc.CANNY_TINY, max_objs=64) == 0 and _create_rc(sc.CANNY_TINY, max_objs=65) == -2
    assert _create_rc(sc.CANNY_TINY, split_weights=1) == -2
    assert _create_rc(sc.CANNY_TINY, extra=60) == 0 and _create_rc(sc.CANNY_TINY, extra=61) == -2 and _create_rc(sc.CANNY_TINY, extra=-1) == -2
    assert _create_rc(sc.CANNY_TINY, grounding=3) == -2
    assert _create_rc(TINY, extra=8) == -2 and _create_rc(TINY, extra=0) == -2          # the entry belongs to the spatial family
    assert _lib.lib().gl_set_extra_channels(None, 8) == -1
    assert _create_rc(dataclasses.replace(TINY, max_objs=65)) == -2 and _create_rc(TINY) == 0


def test_weight_table_and_packer():
    _ensure_built()
    text = dataclasses.replace(TINY, relation=False)
    tables = {}
    for name, cfg in (("canny", sc.CANNY_TINY), ("hed", sc.HED_TINY), ("text", text)):
        h = _lib.create_engine(cfg)
        try:
            tables[name] = _lib.weight_table(h)[0]
        finally:
            _lib.lib().gl_destroy(h)
    for fam in ("canny", "hed"):
        names = [t[0] for t in tables[fam]]
        assert not any(n.startswith(("position_net.", "downsample_net.")) for n in names)
        assert "sd_first_conv.w" in names and "sd_first_conv.b" in names
        assert tables[fam] == [t for t in tables["text"] if not t[0].startswith("position_net.")]       # every slot, the first conv's included
    cfg = sc.CANNY_TINY
    sd = recipe.state_dict(cfg, 0)
    P = weights.pack_state_dict(sd, cfg, "cpu", recipe.sd_first_conv(cfg, 0))
    assert set(P.w) == {t[0] for t in tables["canny"]} and P.has_sd_conv
    w = P.w["input_blocks.0.0.w"].float().reshape(64, 9, 64)                  # [Cout, tap, 64 padded input channels]
    assert float(w[:, :, :12].abs().max()) > 0
    missing = {k: v for k, v in sd.items() if k != "downsample_net.layers.2.bias"}
    with pytest.raises(KeyError, match="missing"):
        weights.pack_state_dict(missing, cfg, "cpu")
    for k in ("position_net.null_feature", "position_net.convnext_tiny_backbone.stages.2.1.gamma"):
        with pytest.raises(KeyError, match=k.replace(".", r"\.")):
            spatial.pack_tokenizer({a: T(np.asarray(b)) for a, b in sd.items() if a != k}, cfg, "cpu")


def test_conditioning_entries_check_the_family():
    _ensure_built()
    l = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    hs, hx = _lib.create_engine(sc.CANNY_TINY), _lib.create_engine(TINY)
    try:
        for rc in (l.gl_set_conditioning(hs, p, p, p, p, p, 1, 77, 10, 16, None), l.gl_set_conditioning_hw(hs, p, p, p, p, p, 1, 77, 10, 16, 16, None),
                   l.gl_set_conditioning_ti(hs, p, p, p, p, p, p, p, p, 1, 77, 10, 16, 16, None), l.gl_set_conditioning_kp(hs, p, p, p, 1, 77, 16, 16, None)):
            assert rc == -1
            assert "grounding = 4 (spatial)" in _lib.last_error(hs) and _lib.last_error(hs).endswith("use gl_set_conditioning_tokens")
        assert l.gl_set_conditioning_tokens(hx, p, p, 1, 77, 16, 16, None) == -1
        e = _lib.last_error(hx)
        assert e.startswith("gl_set_conditioning_tokens:") and "grounding = 0 (text)" in e
        assert l.gl_set_conditioning_tokens(hs, p, p, 1, 77, 16, 20, None) == -1 and "multiples of 8" in _lib.last_error(hs)
        assert l.gl_set_conditioning_tokens(hs, p, p, 1, 77, 16, 16, None) == -1         # the right family, no weights: nothing is read
        assert l.gl_set_conditioning_tokens(None, p, p, 1, 77, 16, 16, None) == -1
        assert l.gl_set_grounding_extra(hx, p, 1, None) == -1 and "no extra channels" in _lib.last_error(hx)
        assert l.gl_set_grounding_extra(hs, p, 1, None) == -1 and "no conditioning call" in _lib.last_error(hs)
        assert l.gl_set_inpaint_extra(hs, p, 1, None) == -1 and "inpaint_mode = 0" in _lib.last_error(hs)
        assert l.gl_set_grounding_extra(None, p, 1, None) == -1
    finally:
        l.gl_destroy(hs)
        l.gl_destroy(hx)


def test_abi_is_additive():
    _ensure_built()
    l = _lib.lib()
    assert _lib.ABI_VERSION == 15 and l.gl_abi_version() == 15
    assert ctypes.sizeof(_lib.UNetConfigC) == l.gl_sizeof_unet_config()
    for fn in ("gl_set_conditioning_tokens", "gl_set_grounding_extra", "gl_set_extra_channels", "gl_sp_stem_patchify", "gl_sp_layernorm", "gl_sp_dwconv_ln", "gl_sp_gelu",
               "gl_sp_down_gather", "gl_sp_assemble", "gl_sp_bicubic", "gl_sp_conv4x4s2"):
        assert fn in _lib.PROTOTYPES and hasattr(l, fn)
    assert _lib.GROUNDING_IDS == {"text": 0, "text_image": 1, "keypoint": 2, "spatial": 4}


# ------------------------------------------------------------------------------------------- packing and tables
def test_gamma_fold():
    g = torch.Generator().manual_seed(3)
    C = 96
    gamma, W, b = torch.randn(C, generator=g), torch.randn(C, 4 * C, generator=g) / 20, torch.randn(C, generator=g)
    x = torch.randn(7, 4 * C, generator=g)
    w2, b2 = spatial.fold_gamma(gamma, W, b)
    want = gamma * (x @ W.t() + b)
    assert float((F.linear(x, w2, b2) - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    P = spatial.pack_tokenizer({k: T(np.asarray(v)) for k, v in recipe.state_dict(sc.CANNY_TINY, 0).items()}, sc.CANNY_TINY, "cpu")
    L = P["stages"][0][0]
    assert tuple(L["w1"].shape) == (384, 128) and float(L["w1"][:, 96:].abs().max()) == 0.0 and tuple(L["dw"].shape) == (49, 96)
    assert tuple(P["stem.w"].shape) == (96, 64) and float(P["stem.w"][:, 48:].abs().max()) == 0.0
    assert tuple(P["down.1.w"].shape) == (64, 384) and tuple(P["pos"].shape) == (4, 768)


SIZES = [(128, 64), (512, 64), (96, 64), (64, 128)]


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_nearest_table_is_torchs(n_in, n_out):
    x = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in).expand(1, 1, 2, n_in)
    want = F.interpolate(x, (2, n_out))[0, 0, 0].numpy().astype(np.int32)
    np.testing.assert_array_equal(spatial.nearest_index(n_in, n_out), want)
    np.testing.assert_array_equal(sp_ref.nearest_resize(x[:, :, :1].expand(1, 1, n_in, n_in), n_out)[0, 0, 0].numpy(), want)


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_bicubic_table_is_torchs(n_in, n_out):
    idx, w = spatial.bicubic_table(n_in, n_out)
    assert idx.shape == (n_out, 4) and w.shape == (n_out, 4) and idx.min() >= 0 and idx.max() <= n_in - 1
    np.testing.assert_allclose(w.sum(1), 1.0, atol=1e-6)
    g = torch.Generator().manual_seed(n_in)
    x = torch.rand(1, 1, n_in, n_in, generator=g) * 2 - 1
    want = F.interpolate(x, (n_out, n_out), mode="bicubic")[0, 0].numpy()
    a = x[0, 0].numpy().astype(np.float64)
    rows = (a[idx.reshape(-1)].reshape(n_out, 4, n_in) * w[:, :, None]).sum(1)                 # along y
    got = (rows[:, idx.reshape(-1)].reshape(n_out, n_out, 4) * w[None]).sum(2)                 # along x
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
    # an impulse at every source position: exactly the table's weight lands on the destinations that index it
    e = torch.eye(n_in).view(n_in, 1, 1, n_in).expand(n_in, 1, 4, n_in).contiguous()
    col = F.interpolate(e, (4, n_out), mode="bicubic")[:, 0, 0].numpy()                        # [source, destination]
    dense = np.zeros((n_in, n_out), np.float64)
    for k in range(4):
        np.add.at(dense, (idx[:, k], np.arange(n_out)), w[:, k])
    np.testing.assert_allclose(dense, col, atol=2e-6)


# ------------------------------------------------------------------------------------------- grounding input, model dispatch, the interface
def test_spatial_grounding_net_input_round_trip():
    g = SpatialGroundingNetInput()
    with pytest.raises(AssertionError):
        g.get_null_input()
    batch = {"map": torch.rand(2, 3, 32, 32), "mask": torch.ones(2, 1)}
    out = g.prepare(batch)
    assert tuple(out) == SpatialGroundingNetInput.KEYS == sp_ref.KEYS and all(out[k] is batch[k] for k in out)
    assert g.prepare(batch, None).keys() == out.keys()
    null = g.get_null_input()
    assert {k: tuple(v.shape) for k, v in null.items()} == {"map": (2, 3, 32, 32), "mask": (2,)}
    assert all(float(v.abs().max()) == 0.0 and v.dtype == torch.float32 for v in null.values())
    assert isinstance(grounding_input_for(sc.CANNY_TINY), SpatialGroundingNetInput) and type(grounding_input_for(TINY)) is GroundingNetInput


def test_model_refusals_without_a_device():
    m = UNetModel.from_packed(None, sc.CANNY_TINY, "cpu")
    m.downsampler = object()
    with pytest.raises(ValueError, match="grounding_extra_input"):
        m.grounding_extra_of({})
    with pytest.raises(ValueError, match="16 x 16"):
        m.grounding_extra_of({"grounding_extra_input": 1}, (32, 32))
    assert m.grounding_extra_of({"grounding_extra_input": 1}, (16, 16)) == 1
    m.cfg = sc.HED_TINY
    with pytest.raises(ValueError, match="64 x 64"):
        m.grounding_extra_of({"grounding_extra_input": 1}, (16, 16))
    m.downsampler = None                                   # every other model ignores the key
    assert m.grounding_extra_of({}) is None and m.grounding_extra_of({"grounding_extra_input": 1}) is None
    with pytest.raises(NotImplementedError, match="strict"):
        UNetModel(dataclasses.replace(sc.CANNY_TINY, split_weights=True), {}, device="cpu")


def test_prepare_batch_spatial_matches_the_reference(tmp_path):
    from PIL import Image
    z = np.load(os.path.join(GOLD, "sp_prepare_batch.npz"))
    path = str(tmp_path / "map.png")
    Image.fromarray(sc.test_image()).save(path)
    want = (T(z["map_u8"]).float() / 255 - 0.5) / 0.5
    for key, src in (("canny_image", path), ("hed_image", path), ("depth", Image.open(path)), ("normal", path)):
        out = itf.prepare_batch_spatial({key: src}, batch=2)
        assert tuple(out) == ("map", "mask") and tuple(out["map"].shape) == tuple(z["shape"]) == (2, 3, 512, 512)
        assert out["map"].dtype == torch.float32 and torch.equal(out["map"][0], want) and torch.equal(out["map"][1], want)
        np.testing.assert_array_equal(out["mask"].numpy(), z["mask"])
    assert hashlib.sha256(out["map"].numpy().tobytes()).hexdigest() == str(z["sha256"])
    multi = itf.prepare_batch_spatial({"canny_image": [path, Image.open(path).transpose(Image.FLIP_LEFT_RIGHT)]}, batch=2)
    assert torch.equal(multi["map"][0], want) and not torch.equal(multi["map"][1], want)
    with pytest.raises(ValueError, match="1 grounding maps for a batch of 2"):
        itf.prepare_batch_spatial({"canny_image": [path]}, batch=2)
    with pytest.raises(ValueError, match="needs its map"):
        itf.prepare_batch_spatial({"prompt": "x"}, batch=1)
    with pytest.raises(ValueError, match="more than one"):
        itf.prepare_batch_spatial({"canny_image": path, "depth": path}, batch=1)


def test_interface_refusals():
    """_run refuses before any encoder runs"""
    class _M(UNetModel):
        def __init__(self, cfg):
            self.cfg, self.downsampler = cfg, (object() if cfg.grounding == "spatial" else None)
    sp, tx = (_M(sc.CANNY_TINY), None, None, None, {}), (_M(TINY), None, None, None, {})
    noise = torch.zeros(1, 4, 16, 16)
    a = dict(batch_size=1)
    with pytest.raises(ValueError, match=r"meta\['images'\]"):
        itf.run_one_image(sp, a, dict(prompt="x", canny_image="a.png", images=["b.png"]), noise)
    with pytest.raises(ValueError, match=r"meta\['input_image'\]"):
        itf.run_one_image(sp, a, dict(prompt="x", canny_image="a.png", input_image="b.png"), noise)
    with pytest.raises(ValueError, match=r"meta\['locations'\]"):
        itf.run_one_image(sp, a, dict(prompt="x", canny_image="a.png", locations=[[0.1, 0.1, 0.5, 0.5]], phrases=["a"]), noise)
    with pytest.raises(ValueError, match="needs its map"):
        itf.run_batch_images(sp, a, dict(prompts=["x"]), noise)
    with pytest.raises(ValueError, match="16 x 16"):
        itf.run_one_image(sp, a, dict(prompt="x", canny_image="a.png"), torch.zeros(1, 4, 32, 32))
    with pytest.raises(ValueError, match="64 x 64"):
        itf.run_one_image((_M(sc.HED_TINY), None, None, None, {}), a, dict(prompt="x", hed_image="a.png"), noise)
    with pytest.raises(ValueError, match="given to a text checkpoint"):
        itf.run_one_image(tx, a, dict(prompt="x", depth="a.png", locations=[], phrases=[]), noise)


def _write_ckpt(path, cfg, family, extra_tensors=()):
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    for k in extra_tensors:
        sd[k] = torch.zeros(1)
    t, d = sc.targets(family)
    config = {"model": {"params": dict(image_size=16, model_channels=64, num_heads=4,
                                       grounding_tokenizer={"target": t, "params": {"resize_input": cfg.sp_resize_input, "out_dim": 768}},
                                       grounding_downsampler={"target": d, "params": {"resize_input": cfg.ds_resize_input, "out_dim": cfg.ds_out}})}}
    torch.save({"model": sd, "config_dict": {"_content": config}}, path)


def test_load_ckpt_refusals(tmp_path, monkeypatch):
    path = str(tmp_path / "canny.pth")
    rela = next(k for k in arch.param_shapes(TINY) if ".rela_fuse." in k)
    _write_ckpt(path, sc.CANNY_TINY, "canny", [rela])
    with pytest.raises(NotImplementedError, match="rela_fuse"):
        itf.load_ckpt(path, "cpu")
    _write_ckpt(path, sc.CANNY_TINY, "canny")
    with pytest.raises(NotImplementedError, match="strict"):
        itf.load_ckpt(path, "cpu", strict=True)
    monkeypatch.setenv("GLIGEN_STRICT", "1")
    with pytest.raises(NotImplementedError, match="strict"):
        itf.load_ckpt(path, "cpu")
    monkeypatch.delenv("GLIGEN_STRICT")

    class _M:
        cfg = sc.CANNY_TINY
    monkeypatch.setattr(itf, "load_all_models", lambda *a, **k: (_M(), None, None, None, {}))
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda *a, **k: 0)
    with pytest.raises(NotImplementedError, match="spatial checkpoint"):
        itf.load_all_models_sharded(path, "cpu")


# ------------------------------------------------------------------------------------------- tests/sp_ref.py vs the reference
_SD = {}


def sp_sd(cfg):
    if cfg not in _SD:
        _SD[cfg] = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    return _SD[cfg]


PIECES = sc.POSNET_CASES + sc.DS_CASES


@pytest.mark.parametrize("case", PIECES, ids=[c["name"] for c in PIECES])
def test_sp_ref_matches_reference(case):
    """the tokenizer and the downsamplers, fp32 against the reference's own fp32 output: rtol 1e-5 / atol 1e-6 (the tolerance of
    tests/test_kp_host.py)"""
    cfg = sc.cfg_of(case)
    inp = {a: T(v) for a, v in sc.case_inputs(case).items()}
    z = np.load(os.path.join(GOLD, case["name"] + ".npz"))
    with torch.no_grad():
        if case["kind"] == "position_net":
            sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="position_net.").items()}
            out = sp_ref.position_net(sd, cfg, inp["map"], inp["mask"])
            ref = z["out_canny"]
            for f in (FAMS if case["name"] == "sp_posnet_t4" else ()):
                np.testing.assert_array_equal(z["out_" + f], ref)           # the four PositionNet classes are one computation
        else:
            sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="downsample_net.").items()}
            out, ref = sp_ref.downsampler(sd, cfg, inp["map"]), z["out"]
    assert out.shape == ref.shape
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", sc.UNET_CASES, ids=[c["name"] for c in sc.UNET_CASES])
def test_sp_ref_unet_matches_reference(case):
    """openaimodel_original.UNetModel with a downsampler.  What tests/sp_ref.py itself states -- the grounding tokens inside the model and the
    first conv on cat([x, downsampler(extra)]) (or the SD conv on x alone) -- is held to rtol 1e-5 / atol 1e-6 against the tensors the
    reference model produced there (``objs``, ``h0``).  Behind the first conv runs oracle/unet_ref.py under tests/norel_ref.py, and the
    transformer blocks amplify the last-bit differences of two fp32 evaluations: 6.6e-7 in the tokens (T = 4: torch's Linear on 8 rows is not
    bitwise repeatable between the module and the functional call) become 5.3e-6 in the output of the 16 x 16 cases, and the 64 x 64 hed
    cases differ by 4.3e-6 even on the SD conv at fuser scale 0, where neither tokens nor the extra enter (max |diff| / (1e-6 + 1e-5 |ref|)
    = 3.5 and 3.2).  The whole output is therefore held to a relative L2 of 1e-5 instead: fp32 unit roundoff 6e-8 over the ~600 sequential
    roundings of the tiny UNet (6e-8 * sqrt(600) = 1.5e-6) with a margin of 7 for the softmax / GroupNorm amplification."""
    cfg = sc.cfg_of(case)
    inp = {a: T(v) for a, v in sc.case_inputs(case).items()}
    z = np.load(os.path.join(GOLD, case["name"] + ".npz"))
    sd = sp_sd(cfg)
    fc = {a: T(v) for a, v in recipe.sd_first_conv(cfg, 0).items()} if case["sdconv"] else None
    g, ctx = {k: inp[k] for k in sp_ref.KEYS}, inp["context"]
    if case["grounding"] == "null":
        g, ctx = sp_ref.null_grounding(g), inp["uc"]
    s = sc.h0_stride(case)
    with torch.no_grad():
        objs = sp_ref.position_net(sd, cfg, g["map"], g["mask"])
        h0 = sp_ref.first_conv_out(sd, cfg, inp["x"], inp["map"], fc)[:, :, ::s, ::s]
        out = sp_ref.unet_forward(sd, cfg, inp["x"], torch.tensor(case["t"]), ctx, g, inp["map"], fuser_scale=case["scale"], first_conv=fc)
    assert objs.shape == z["objs"].shape and h0.shape == z["h0"].shape and out.shape == z["out"].shape
    np.testing.assert_allclose(objs.numpy(), z["objs"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(h0.numpy(), z["h0"], rtol=1e-5, atol=1e-6)
    r = float(np.linalg.norm(out.numpy() - z["out"]) / np.linalg.norm(z["out"]))
    print(f"[{case['name']}] whole output rel_l2 = {r:.2e}, max |diff| = {np.abs(out.numpy() - z['out']).max():.2e}")
    assert r < 1e-5, r


def test_goldens_see_their_inputs():
    case = sc.by_name("sp_posnet_t4")
    cfg = sc.cfg_of(case)
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="position_net.").items()}
    inp = {a: T(v) for a, v in sc.case_inputs(case).items()}
    ref = np.load(os.path.join(GOLD, "sp_posnet_t4.npz"))["out_canny"]
    assert inp["mask"].tolist() == [1.0, 0.0]
    null = sp_ref.position_net(sd, cfg, torch.zeros_like(inp["map"]), torch.zeros(2)).numpy()
    np.testing.assert_allclose(ref[1], null[1], rtol=1e-5, atol=1e-6)                     # the masked-out sample: the null tokens
    assert np.abs(ref[0] - null[0]).max() > 1e-2                                          # the other one sees its map ...
    assert np.abs(sp_ref.position_net(sd, cfg, inp["map"].flip(-1), inp["mask"]).numpy()[0] - ref[0]).max() > 1e-3      # ... and where things are
    for k in ("position_net.pos_embedding", "position_net.convnext_tiny_backbone.stages.0.0.gamma"):
        rolled = {**sd, k: torch.roll(sd[k], 1, -2 if k.endswith("pos_embedding") else 0)}
        assert np.abs(sp_ref.position_net(rolled, cfg, inp["map"], inp["mask"]).numpy()[0] - ref[0]).max() > 1e-3, k
    real, null_, s0 = (np.load(os.path.join(GOLD, n + ".npz"))["out"] for n in ("sp_unet_canny_s1", "sp_unet_canny_null", "sp_unet_canny_s0_sd"))
    assert np.linalg.norm(real - null_) / np.linalg.norm(null_) > 1e-2
    # canny, depth and normal differ: the channels they read and their own weights' names are the same, the inputs are not
    ds = {f: np.load(os.path.join(GOLD, f"sp_ds_{f}.npz"))["out"] for f in ("canny", "depth", "normal")}
    assert np.abs(ds["canny"] - ds["normal"]).max() > 1e-2
