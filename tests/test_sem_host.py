"""CPU tests (no GPU) of the semantic-map grounding family (GLIGEN's checkpoint_generation_sem.pth): config parsing with and without
``allow_semantic`` and the refusals that stay, parameter names against the reference's, gl_create on a sem config, the new prototypes at ABI
15, the gather table, prepare_batch_sem against the reference's own batch, the interface's refusals, a synthetic checkpoint through load_ckpt's
parsing, and tests/sem_ref.py against the reference's own outputs (tests/golden/sem_*.npz)."""
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
import sem_cases as sm
import sem_ref
import sp_cases as sc
from layoutllm_t2i_amd import _lib, arch, recipe, semantic
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY, UNetConfig
from layoutllm_t2i_amd.model import SemGroundingNetInput, SpatialGroundingNetInput, UNetModel, grounding_input_for

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
HEADER = os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "gligen_hip.h")
NEW_ENTRIES = ("gl_sem_gather_conv", "gl_sem_conv4x4s2", "gl_sem_onehot_index")


def _ensure_built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)


def _params(tok=None, ds=None, classes=152, ds_classes=None, resize=256, **kw):
    t, d = sm.targets()
    return {"model_channels": 64, "num_heads": 4, **kw,
            "grounding_tokenizer": {"target": tok or t, "params": {"in_dim": classes, "resize_input": resize, "out_dim": 768}},
            "grounding_downsampler": {"target": ds or d, "params": {"in_dim": classes if ds_classes is None else ds_classes, "resize_input": 256,
                                                                    "out_dim": 8}}}


# ------------------------------------------------------------------------------------------- configuration
def test_from_dict_with_the_flag():
    cfg = UNetConfig.from_dict(_params(), allow_semantic=True)
    assert cfg.grounding == "spatial" and cfg.ds_kind == "sem" and cfg.relation is False
    assert (cfg.ds_in, cfg.sem_classes, cfg.ds_out, cfg.first_conv_in) == (152, 152, 8, 12)
    assert cfg.n_ground == 64 == cfg.max_objs and cfg.sp_resize_input == 256 and cfg.ds_resize_input == 256 and cfg.ds_latent == 64
    assert cfg.pos_in_dim == 768 and cfg.pos_out_dim == 768                  # in_dim counts classes: it is no embedding width
    c = _lib.unet_config_c(cfg)
    assert c.grounding == 4 and c.max_objs == 64 and c.no_relation == 1
    assert cfg == UNetConfig.from_dict(_params(), allow_semantic=True, allow_spatial=True, allow_inpaint=True, allow_keypoint=True)
    assert UNetConfig.from_dict(_params(classes=5, resize=64), allow_semantic=True).sem_classes == 5
    assert UNetConfig.from_dict(_params(resize=64), allow_semantic=True).n_ground == 4
    assert TINY.sem_classes == 0 and sc.CANNY_TINY.sem_classes == 0
    assert "sem_grounding_net" not in arch.SPATIAL_FAMILIES and len(arch.SPATIAL_FAMILIES) == 4


def test_from_dict_refusals():
    sem_t, sem_d = sm.targets()
    canny_t, canny_d = sc.targets("canny")
    for kw in ({}, dict(allow_spatial=True), dict(allow_spatial=True, allow_inpaint=True, allow_keypoint=True)):      # without the flag: as before
        with pytest.raises(NotImplementedError, match="grounding_downsampler"):
            UNetConfig.from_dict(_params(), **kw)
    bad = [
        _params(ds=canny_d),                                                  # the sem tokenizer with another family's downsampler
        _params(ds="x"),
        _params(tok=canny_t),                                                 # a canny tokenizer with the sem downsampler
        _params(inpaint_mode=True),
        {k: v for k, v in _params().items() if k != "grounding_downsampler"},                 # the tokenizer without its downsampler
        {"grounding_downsampler": _params()["grounding_downsampler"]},                        # the downsampler on a text tokenizer
    ]
    for p in bad:
        for kw in (dict(allow_semantic=True), dict(allow_semantic=True, allow_spatial=True, allow_inpaint=True)):
            with pytest.raises(NotImplementedError, match="grounding_downsampler"):
                UNetConfig.from_dict(p, **kw)
    with pytest.raises(ValueError, match="resize_input"):                     # 196 tokens: over the fuser's 64
        UNetConfig.from_dict(_params(resize=448), allow_semantic=True)
    with pytest.raises(ValueError, match="in_dim"):                           # the two in_dims are one number
        UNetConfig.from_dict(_params(ds_classes=150), allow_semantic=True)
    for c in (1, 257):
        with pytest.raises(ValueError, match="2 .. 256"):
            UNetConfig.from_dict(_params(classes=c), allow_semantic=True)
    assert UNetConfig.from_dict(_params(classes=256), allow_semantic=True).sem_classes == 256
    base = {"model_channels": 64, "num_heads": 4}
    assert UNetConfig.from_dict(base) == UNetConfig.from_dict(base, allow_semantic=True)
    canny = {**base, "grounding_tokenizer": {"target": canny_t, "params": {"resize_input": 256, "out_dim": 768}},
             "grounding_downsampler": {"target": canny_d, "params": {"resize_input": 256, "out_dim": 8}}}
    assert UNetConfig.from_dict(canny, allow_spatial=True) == UNetConfig.from_dict(canny, allow_spatial=True, allow_semantic=True)
    with pytest.raises(NotImplementedError, match="grounding_downsampler"):                   # the sem flag does not open the canny family
        UNetConfig.from_dict(canny, allow_semantic=True)


def test_param_shapes_match_the_reference_model():
    z = np.load(os.path.join(GOLD, "sem_params.npz"))
    want = {str(n): tuple(int(v) for v in str(s).split(",")) if str(s) else () for n, s in zip(z["names"], z["shapes"])}
    got = arch.param_shapes(sm.SEM_TINY)
    assert got == want and list(got) == [str(n) for n in z["names"]]          # names, shapes and the state dict's order
    assert got["position_net.in_conv.weight"] == (3, 152, 3, 3) and got["position_net.in_conv.bias"] == (3,)
    assert got["downsample_net.layers.0.weight"] == (16, 152, 4, 4) and got["downsample_net.layers.2.weight"] == (8, 16, 4, 4)
    assert got["input_blocks.0.0.weight"] == (64, 12, 3, 3)
    canny = arch.param_shapes(sc.CANNY_TINY)
    own = ("position_net.in_conv.", "downsample_net.")
    assert {k: v for k, v in got.items() if not k.startswith(own)} == {k: v for k, v in canny.items() if not k.startswith(own)}     # the rest as canny
    assert list(recipe.state_dict(sm.SEM_TINY, 0)) == list(got)
    assert arch.param_shapes(sm.sem_cfg(TINY, 64, classes=5))["position_net.in_conv.weight"] == (3, 5, 3, 3)


# ------------------------------------------------------------------------------------------- the library
def test_gl_create_on_a_sem_config():
    _ensure_built()
    l = _lib.lib()
    cc, h = _lib.unet_config_c(sm.SEM_TINY), ctypes.c_void_p()
    assert l.gl_create(ctypes.byref(cc), ctypes.byref(h)) == 0
    try:
        assert l.gl_set_extra_channels(h, 8) == 0
    finally:
        l.gl_destroy(h)
    h = _lib.create_engine(sm.SEM_TINY)
    try:
        names = [t[0] for t in _lib.weight_table(h)[0]]
        assert not any(n.startswith(("position_net.", "downsample_net.")) for n in names) and "sd_first_conv.w" in names
    finally:
        l.gl_destroy(h)


def test_new_entries_are_additive_at_abi_15():
    _ensure_built()
    l = _lib.lib()
    assert _lib.ABI_VERSION == 15 and l.gl_abi_version() == 15
    assert ctypes.sizeof(_lib.UNetConfigC) == l.gl_sizeof_unet_config()
    assert _lib.GROUNDING_IDS == {"text": 0, "text_image": 1, "keypoint": 2, "spatial": 4}
    header = open(HEADER).read()
    for fn in NEW_ENTRIES:
        assert fn in _lib.PROTOTYPES and hasattr(l, fn) and f"int {fn}(" in header
    assert len(_lib.PROTOTYPES["gl_sem_gather_conv"][1]) == 15 and len(_lib.PROTOTYPES["gl_sem_conv4x4s2"][1]) == 10
    assert len(_lib.PROTOTYPES["gl_sem_onehot_index"][1]) == 8


def test_bad_arguments_are_refused_before_any_launch():
    """GL_ERR_BAD_ARG by return code, without a device: every check comes before the launch"""
    _ensure_built()
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    a = p + (-p % 16)                                                        # a 16-byte aligned address inside the buffer
    ok = dict(map=a, B=1, Hs=8, Ws=8, R=8, table=a, bias=a, classes=152, K=4, stride=2, pad=1, Co=16, silu=1, out=a)

    def gather(**kw):
        v = {**ok, **kw}
        return l.gl_sem_gather_conv(v["map"], v["B"], v["Hs"], v["Ws"], v["R"], v["table"], v["bias"], v["classes"], v["K"], v["stride"], v["pad"],
                                    v["Co"], v["silu"], v["out"], None)
    for kw in (dict(map=None), dict(table=None), dict(bias=None), dict(out=None), dict(classes=1), dict(classes=257), dict(Co=17), dict(Co=0),
               dict(R=7), dict(B=0), dict(K=5), dict(stride=3), dict(pad=4), dict(table=a + 4), dict(B=1 << 20, R=1 << 15)):
        assert gather(**kw) == -1, kw
    assert l.gl_sem_conv4x4s2(None, a, a, 1, 16, 8, 8, 8, a, None) == -1 and l.gl_sem_conv4x4s2(a, a, a, 1, 16, 8, 7, 8, a, None) == -1
    assert l.gl_sem_conv4x4s2(a, a, a, 1, 65, 8, 8, 8, a, None) == -1 and l.gl_sem_conv4x4s2(a, a, a, 1, 16, 0, 8, 8, a, None) == -1
    assert l.gl_sem_onehot_index(None, 1, 152, 8, 8, a, a, None) == -1 and l.gl_sem_onehot_index(a, 1, 257, 8, 8, a, a, None) == -1
    assert l.gl_sem_onehot_index(a, 1, 1, 8, 8, a, a, None) == -1 and l.gl_sem_onehot_index(a, 1, 152, 8, 8, a, None, None) == -1


def test_gather_table_is_the_conv():
    """table[class][tap][co] summed over the taps of a pixel == F.conv2d of the one-hot (interior and border), in float64"""
    g = torch.Generator().manual_seed(5)
    C, Co, K = 7, 3, 3
    w, b = torch.randn(Co, C, K, K, generator=g).double(), torch.randn(Co, generator=g).double()
    t = semantic.gather_table(w.float()).double()
    assert tuple(t.shape) == (C, 9, 4) and float(t[:, :, 3].abs().max()) == 0.0
    cm = torch.randint(0, C, (1, 6, 5), generator=g)
    want = F.conv2d(sem_ref.onehot(cm, C).double(), w, b, padding=1)
    got = b.view(1, Co, 1, 1).repeat(1, 1, 6, 5).clone()
    for y in range(6):
        for x in range(5):
            for ky in range(3):
                for kx in range(3):
                    sy, sx = y - 1 + ky, x - 1 + kx
                    if 0 <= sy < 6 and 0 <= sx < 5:
                        got[0, :, y, x] += t[cm[0, sy, sx], ky * 3 + kx, :Co]
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
    assert tuple(semantic.gather_table(torch.zeros(16, 152, 4, 4)).shape) == (152, 16, 16)        # 155 648 bytes


# ------------------------------------------------------------------------------------------- grounding input, the interface
def test_sem_grounding_net_input_round_trip():
    g = SemGroundingNetInput()
    with pytest.raises(AssertionError):
        g.get_null_input()
    assert SemGroundingNetInput.KEYS == ("sem", "mask") == sem_ref.KEYS and SpatialGroundingNetInput.KEYS == ("map", "mask")
    for sem in (torch.zeros(2, 32, 32, dtype=torch.uint8), torch.zeros(2, 5, 32, 32)):        # both input forms
        batch = {"sem": sem, "mask": torch.ones(2, 1)}
        out = g.prepare(batch)
        assert tuple(out) == ("sem", "mask") and all(out[k] is batch[k] for k in out)
        null = g.get_null_input()
        assert null["sem"].shape == sem.shape and null["sem"].dtype == sem.dtype and tuple(null["mask"].shape) == (2,)
        assert float(null["sem"].float().abs().max()) == 0.0 and float(null["mask"].abs().max()) == 0.0 and null["mask"].dtype == torch.float32
    assert type(grounding_input_for(sm.SEM_TINY)) is SemGroundingNetInput
    assert type(grounding_input_for(sc.CANNY_TINY)) is SpatialGroundingNetInput


def test_prepare_batch_sem_matches_the_reference(tmp_path):
    from PIL import Image
    z = np.load(os.path.join(GOLD, "sem_prepare_batch.npz"))
    path = str(tmp_path / "sem.png")
    Image.fromarray(sm.test_image(), "L").save(path)
    want = T(z["map_u8"])
    assert tuple(z["shape"]) == (2, 152, 512, 512) and int(want.min()) == 0 and int(want.max()) == 151
    for src in (path, Image.open(path)):
        out = itf.prepare_batch_sem({"sem": src}, 2)
        assert tuple(out) == ("sem", "mask") and out["sem"].dtype == torch.uint8 and tuple(out["sem"].shape) == (2, 512, 512)
        assert torch.equal(out["sem"][0], want) and torch.equal(out["sem"][1], want)
        np.testing.assert_array_equal(out["mask"].numpy(), z["mask"])
    # the reference's own tensor is the one-hot of this map: the same bytes (one sample at a time: 159 MB each)
    h = hashlib.sha256()
    for b in range(2):
        h.update(sem_ref.onehot(out["sem"][b:b + 1], 152).numpy().tobytes())
    assert h.hexdigest() == str(z["sha256"])
    multi = itf.prepare_batch_sem({"sem": [path, Image.open(path).transpose(Image.FLIP_LEFT_RIGHT)]}, 2)
    assert torch.equal(multi["sem"][0], want) and torch.equal(multi["sem"][1], want.flip(-1))
    with pytest.raises(ValueError, match="1 semantic maps for a batch of 2"):
        itf.prepare_batch_sem({"sem": [path]}, 2)
    with pytest.raises(ValueError, match="needs its class map"):
        itf.prepare_batch_sem({"prompt": "x"}, 1)
    with pytest.raises(ValueError, match="class id 151"):                     # the reference's scatter_ raises there too
        itf.prepare_batch_sem({"sem": path}, 1, classes=151)
    assert not os.path.exists("sem_vis.png")                                  # the colour visualisation is not written
    assert itf.SPATIAL_META_KEYS == ("canny_image", "hed_image", "depth", "normal") and itf.SEM_META_KEY == "sem"


def test_interface_refusals():
    """_run refuses before any encoder runs (the stub-model technique of test_sp_host.test_interface_refusals)"""
    class _M(UNetModel):
        def __init__(self, cfg):
            self.cfg, self.downsampler = cfg, (object() if cfg.grounding == "spatial" else None)
    se, ca, tx = ((_M(c), None, None, None, {}) for c in (sm.SEM_TINY, sc.CANNY_TINY, TINY))
    noise = torch.zeros(1, 4, 16, 16)
    a = dict(batch_size=1)
    with pytest.raises(ValueError, match=r"meta\['sem'\]\) given to a text checkpoint"):
        itf.run_one_image(tx, a, dict(prompt="x", sem="a.png", locations=[], phrases=[]), noise)
    with pytest.raises(ValueError, match=r"meta\['sem'\]\) given to a canny / hed / depth / normal checkpoint"):
        itf.run_one_image(ca, a, dict(prompt="x", sem="a.png"), noise)
    for key in itf.SPATIAL_META_KEYS:
        with pytest.raises(ValueError, match=f"{key}\\) given to a semantic-map checkpoint"):
            itf.run_one_image(se, a, {"prompt": "x", key: "a.png"}, noise)
    with pytest.raises(ValueError, match=r"meta\['images'\]"):
        itf.run_one_image(se, a, dict(prompt="x", sem="a.png", images=["b.png"]), noise)
    with pytest.raises(ValueError, match=r"meta\['input_image'\]"):
        itf.run_one_image(se, a, dict(prompt="x", sem="a.png", input_image="b.png"), noise)
    with pytest.raises(ValueError, match=r"meta\['locations'\]"):
        itf.run_one_image(se, a, dict(prompt="x", sem="a.png", locations=[[0.1, 0.1, 0.5, 0.5]], phrases=["a"]), noise)
    with pytest.raises(ValueError, match="needs its class map"):
        itf.run_batch_images(se, a, dict(prompts=["x"]), noise)
    with pytest.raises(ValueError, match="16 x 16"):
        itf.run_one_image(se, a, dict(prompt="x", sem="a.png"), torch.zeros(1, 4, 32, 32))


def _write_ckpt(path, cfg, extra_tensors=()):
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    for k in extra_tensors:
        sd[k] = torch.zeros(1)
    t, d = sm.targets()
    config = {"model": {"params": dict(image_size=16, model_channels=64, num_heads=4,
                                       grounding_tokenizer={"target": t, "params": {"in_dim": cfg.sem_classes, "resize_input": cfg.sp_resize_input,
                                                                                    "out_dim": 768}},
                                       grounding_downsampler={"target": d, "params": {"in_dim": cfg.sem_classes, "resize_input": cfg.ds_resize_input,
                                                                                      "out_dim": cfg.ds_out}})}}
    torch.save({"model": sd, "config_dict": {"_content": config}}, path)


def test_load_ckpt_parses_a_sem_checkpoint_and_keeps_the_spatial_refusals(tmp_path, monkeypatch):
    """a synthetic sem checkpoint is read as the sem family from its config (the file is not named after it): past from_dict, the
    rela_fuse and strict refusals; the sharded entry refuses"""
    path = str(tmp_path / "some_model.pth")
    rela = next(k for k in arch.param_shapes(TINY) if ".rela_fuse." in k)
    _write_ckpt(path, sm.SEM_TINY, [rela])
    with pytest.raises(NotImplementedError, match="rela_fuse"):
        itf.load_ckpt(path, "cpu")
    _write_ckpt(path, sm.SEM_TINY)
    with pytest.raises(NotImplementedError, match="strict"):
        itf.load_ckpt(path, "cpu", strict=True)
    monkeypatch.setenv("GLIGEN_STRICT", "1")
    with pytest.raises(NotImplementedError, match="strict"):
        itf.load_ckpt(path, "cpu")
    monkeypatch.delenv("GLIGEN_STRICT")
    with pytest.raises(NotImplementedError, match="strict"):
        UNetModel(dataclasses.replace(sm.SEM_TINY, split_weights=True), {}, device="cpu")

    class _M:
        cfg = sm.SEM_TINY
    monkeypatch.setattr(itf, "load_all_models", lambda *a, **k: (_M(), None, None, None, {}))
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda *a, **k: 0)
    with pytest.raises(NotImplementedError, match="spatial checkpoint"):
        itf.load_all_models_sharded(path, "cpu")


# ------------------------------------------------------------------------------------------- tests/sem_ref.py vs the reference
_SD = {}


def sem_sd(cfg):
    if cfg not in _SD:
        _SD[cfg] = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    return _SD[cfg]


PIECES = sm.POSNET_CASES + sm.DS_CASES


def test_case_maps_hold_the_first_and_the_last_class():
    for case in sm.CASES:
        if "S" in case:
            m = sm.case_inputs(case)["sem"]
            assert m.dtype == np.uint8 and m.min() == 0 and m.max() == case["classes"] - 1
            assert len(np.unique(m)) == case["classes"]                       # random over all classes
    t = sm.test_image()
    assert t.shape == (64, 96) and 0 in t[:, 16:80] and 151 in t[:, 16:80]


@pytest.mark.parametrize("case", PIECES, ids=[c["name"] for c in PIECES])
def test_sem_ref_matches_reference(case):
    """the tokenizer (152 and 5 classes) and the downsampler, fp32 against the reference's own fp32 output: rtol 1e-5 / atol 1e-6"""
    cfg = sm.cfg_of(case)
    inp = {a: T(v) for a, v in sm.case_inputs(case).items()}
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    with torch.no_grad():
        if case["kind"] == "position_net":
            sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="position_net.").items()}
            out = sem_ref.position_net(sd, cfg, inp["sem"], inp["mask"])
        else:
            sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="downsample_net.").items()}
            out = sem_ref.downsampler(sd, cfg, inp["sem"])
    assert out.shape == ref.shape
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", sm.UNET_CASES, ids=[c["name"] for c in sm.UNET_CASES])
def test_sem_ref_unet_matches_reference(case):
    """openaimodel_original.UNetModel with the sem tokenizer and downsampler.  The tokens and the first conv's output, which tests/sem_ref.py
    itself states, are held to rtol 1e-5 / atol 1e-6; the whole output to a relative L2 of 1e-5, the bound and the reasoning of
    tests/test_sp_host.py::test_sp_ref_unet_matches_reference (behind the first conv runs the same oracle, and the transformer blocks
    amplify the last-bit differences of two fp32 evaluations)."""
    cfg = sm.cfg_of(case)
    inp = {a: T(v) for a, v in sm.case_inputs(case).items()}
    z = np.load(os.path.join(GOLD, case["name"] + ".npz"))
    sd = sem_sd(cfg)
    fc = {a: T(v) for a, v in recipe.sd_first_conv(cfg, 0).items()} if case["sdconv"] else None
    g, ctx = {k: inp[k] for k in sem_ref.KEYS}, inp["context"]
    if case["grounding"] == "null":
        g, ctx = sem_ref.null_grounding(g), inp["uc"]
    with torch.no_grad():
        objs = sem_ref.position_net(sd, cfg, g["sem"], g["mask"])
        h0 = sem_ref.first_conv_out(sd, cfg, inp["x"], inp["sem"], fc)
        out = sem_ref.unet_forward(sd, cfg, inp["x"], torch.tensor(case["t"]), ctx, g, inp["sem"], fuser_scale=case["scale"], first_conv=fc)
    assert objs.shape == z["objs"].shape and h0.shape == z["h0"].shape and out.shape == z["out"].shape
    np.testing.assert_allclose(objs.numpy(), z["objs"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(h0.numpy(), z["h0"], rtol=1e-5, atol=1e-6)
    r = float(np.linalg.norm(out.numpy() - z["out"]) / np.linalg.norm(z["out"]))
    print(f"[{case['name']}] whole output rel_l2 = {r:.2e}, max |diff| = {np.abs(out.numpy() - z['out']).max():.2e}")
    assert r < 1e-5, r


def test_goldens_see_their_inputs():
    case = sm.by_name("sem_posnet_c152")
    cfg = sm.cfg_of(case)
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="position_net.").items()}
    inp = {a: T(v) for a, v in sm.case_inputs(case).items()}
    ref = np.load(os.path.join(GOLD, "sem_posnet_c152.npz"))["out"]
    null = sem_ref.position_net(sd, cfg, torch.zeros_like(inp["sem"]), torch.zeros(2)).numpy()
    np.testing.assert_allclose(ref[1], null[1], rtol=1e-5, atol=1e-6)                     # the masked-out sample: the null tokens
    assert np.abs(ref[0] - null[0]).max() > 1e-2                                          # the other one sees its map ...
    assert np.abs(sem_ref.position_net(sd, cfg, inp["sem"].flip(-1), inp["mask"]).numpy()[0] - ref[0]).max() > 1e-3      # ... and where things are
    rolled = {**sd, "position_net.in_conv.weight": torch.roll(sd["position_net.in_conv.weight"], 1, 1)}                  # ... and which class is which
    assert np.abs(sem_ref.position_net(rolled, cfg, inp["sem"], inp["mask"]).numpy()[0] - ref[0]).max() > 1e-3
    real, null_ = (np.load(os.path.join(GOLD, n + ".npz"))["out"] for n in ("sem_unet_s1", "sem_unet_null"))
    assert np.linalg.norm(real - null_) / np.linalg.norm(null_) > 1e-2
    assert np.abs(ref - np.load(os.path.join(GOLD, "sem_posnet_c5.npz"))["out"])[0].max() > 1e-3
