"""CPU tests (no GPU) of the text_image grounding family (GLIGEN's *_box_text_image checkpoints): config parsing, the engine's weight
table against the packer, the token-count limit, the family check of the conditioning entries, the grounding-tokenizer input, the
image branch of prepare_batch with stub CLIP objects, and tests/ti_ref.py against the reference's own outputs (tests/golden/ti_*.npz)."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ti_cases as tc
import ti_ref
from layoutllm_t2i_amd import _lib, arch, recipe, weights
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY, UNetConfig
from layoutllm_t2i_amd.model import GroundingNetInput, TextImageGroundingNetInput, grounding_input_for

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
TI_TARGET = "ldm.modules.diffusionmodules.text_image_grounding_net.PositionNet"
TEXT_TARGET = "ldm.modules.diffusionmodules.text_grounding_net.PositionNet"
PN_NAMES = ["position_net.null_text", "position_net.null_image", "position_net.null_xyxy"] + [
    f"position_net.{c}.{i}.{s}" for c in ("linears_text", "linears_image") for i in (0, 2, 4) for s in ("w", "b")]


def _ensure_built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)


# ------------------------------------------------------------------------------------------- configuration
def test_from_dict_selects_the_grounding_family():
    base = dict(model_channels=64, num_heads=4)
    ti = UNetConfig.from_dict({**base, "grounding_tokenizer": {"target": TI_TARGET, "params": {"in_dim": 768, "out_dim": 768}}})
    assert ti.grounding == "text_image" and ti.n_ground == 60 and dataclasses.replace(ti, image_size=16) == tc.TI_TINY
    assert dataclasses.replace(ti, grounding="text", image_size=16) == TINY
    tx = UNetConfig.from_dict({**base, "grounding_tokenizer": {"target": TEXT_TARGET, "params": {}}})
    assert tx.grounding == "text" and tx.n_ground == 30
    assert UNetConfig.from_dict(base).grounding == "text" and UNetConfig().grounding == "text"
    with pytest.raises(NotImplementedError, match="keypoint"):
        UNetConfig.from_dict({**base, "grounding_tokenizer": {"target": "ldm.modules.diffusionmodules.keypoint_grounding_net.PositionNet"}})


def test_param_shapes_of_both_families():
    tx, ti = arch.param_shapes(TINY), arch.param_shapes(tc.TI_TINY)
    body = lambda d: {k: v for k, v in d.items() if not k.startswith("position_net.")}
    assert body(tx) == body(ti)
    pn = {k: v for k, v in ti.items() if k.startswith("position_net.")}
    want = {"position_net.null_text_feature": (768,), "position_net.null_image_feature": (768,), "position_net.null_position_feature": (64,)}
    for c in ("linears_text", "linears_image"):
        want.update({f"position_net.{c}.0.weight": (512, 832), f"position_net.{c}.0.bias": (512,), f"position_net.{c}.2.weight": (512, 512),
                     f"position_net.{c}.2.bias": (512,), f"position_net.{c}.4.weight": (768, 512), f"position_net.{c}.4.bias": (768,)})
    assert pn == want
    assert "position_net.linears.0.weight" in tx and "position_net.null_positive_feature" in tx


@pytest.mark.parametrize("split", [False, True], ids=["compact", "split"])
def test_weight_table_equals_the_packer(split):
    """the gl_create table of TINY text_image: the text table's names with the PositionNet entries replaced, shapes as the packer fills
    them (compact: [N, K]; split_weights: [N, 2 K] = [Whi | Wlo])"""
    _ensure_built()
    cfg = dataclasses.replace(tc.TI_TINY, split_weights=split)
    h = _lib.create_engine(cfg)
    ht = _lib.create_engine(dataclasses.replace(TINY, split_weights=split))
    try:
        table, total = _lib.weight_table(h)
        text_table, _ = _lib.weight_table(ht)
    finally:
        _lib.lib().gl_destroy(h)
        _lib.lib().gl_destroy(ht)
    names = [t[0] for t in table]
    assert [n for n in names if n.startswith("position_net.")] == PN_NAMES
    assert [n for n in names if not n.startswith("position_net.")] == [t[0] for t in text_table if not t[0].startswith("position_net.")]
    shapes = {t[0]: t[4] for t in table}
    k = 2 if split else 1
    for c in ("linears_text", "linears_image"):
        assert shapes[f"position_net.{c}.0.w"] == (512, 832 * k) and shapes[f"position_net.{c}.2.w"] == (512, 512 * k)
        assert shapes[f"position_net.{c}.4.w"] == (768, 512 * k) and shapes[f"position_net.{c}.4.b"] == (768,)
    assert shapes["position_net.null_text"] == (768,) and shapes["position_net.null_image"] == (768,) and shapes["position_net.null_xyxy"] == (64,)
    sd = recipe.state_dict(cfg, 0)
    P = weights.pack_state_dict(sd, cfg, "cpu")
    assert P.flat.numel() == total and set(P.w) == set(names)
    for name, off, nbytes, dtype, shape in table:
        assert tuple(P.w[name].shape) == tuple(shape) and P.w[name].data_ptr() == P.flat.data_ptr() + off
    # values: the image chain's first matrix is the fp16 of ITS state-dict tensor (not the text chain's), nulls verbatim
    w = T(sd["position_net.linears_image.0.weight"])
    assert torch.equal(P.w["position_net.linears_image.0.w"][:, :832], w.half())
    if split:
        assert torch.equal(P.w["position_net.linears_image.0.w"][:, 832:], (w - w.half().float()).half())
    assert torch.equal(P.w["position_net.null_image"], T(sd["position_net.null_image_feature"]))
    assert torch.equal(P.w["position_net.null_text"], T(sd["position_net.null_text_feature"]))
    # a text-family state dict does not load into a text_image config
    with pytest.raises(KeyError, match="missing"):
        weights.pack_state_dict(recipe.state_dict(TINY, 0), cfg, "cpu")


def test_default_table_is_unchanged():
    _ensure_built()
    h = _lib.create_engine(UNetConfig())
    try:
        table, _ = _lib.weight_table(h)
    finally:
        _lib.lib().gl_destroy(h)
    assert len(table) == 1102 and not any("linears_text" in t[0] or "null_text" in t[0] for t in table)
    assert _lib.unet_config_c(UNetConfig()).grounding == 0 and _lib.unet_config_c(tc.TI_TINY).grounding == 1
    assert ctypes.sizeof(_lib.UNetConfigC) == _lib.lib().gl_sizeof_unet_config()


def test_token_count_limit():
    """gl_create: n_ground = max_objs (text) or 2 * max_objs (text_image) must not exceed 64"""
    _ensure_built()
    l = _lib.lib()
    for cfg, ok in ((dataclasses.replace(tc.TI_TINY, max_objs=32), True), (dataclasses.replace(tc.TI_TINY, max_objs=33), False),
                    (dataclasses.replace(TINY, max_objs=64), True), (dataclasses.replace(TINY, max_objs=65), False)):
        cc, h = _lib.unet_config_c(cfg), ctypes.c_void_p()
        rc = l.gl_create(ctypes.byref(cc), ctypes.byref(h))
        assert (rc == 0) == ok, (cfg.grounding, cfg.max_objs, rc)
        if rc == 0:
            l.gl_destroy(h)
    cc, h = _lib.unet_config_c(TINY), ctypes.c_void_p()
    cc.grounding = 2
    assert l.gl_create(ctypes.byref(cc), ctypes.byref(h)) != 0


def test_conditioning_entries_check_the_family():
    """the text entries on a text_image handle and gl_set_conditioning_ti on a text handle return GL_ERR_BAD_ARG (-1) before they read any
    argument: no GPU, no weights, dangling-free dummy pointers"""
    _ensure_built()
    l = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    hti, htx = _lib.create_engine(tc.TI_TINY), _lib.create_engine(TINY)
    try:
        assert _lib.last_error(hti) == "" and _lib.last_error(htx) == ""
        assert l.gl_set_conditioning(hti, p, p, p, p, p, 1, 77, 10, 16, None) == -1
        assert _lib.last_error(hti).startswith("gl_set_conditioning:") and "grounding = 1 (text_image)" in _lib.last_error(hti)
        assert "gl_set_conditioning_ti" in _lib.last_error(hti)
        assert l.gl_set_conditioning_hw(hti, p, p, p, p, p, 1, 77, 10, 16, 24, None) == -1
        assert _lib.last_error(hti).startswith("gl_set_conditioning_hw:") and "grounding = 1 (text_image)" in _lib.last_error(hti)
        assert l.gl_set_conditioning_ti(htx, p, p, p, p, p, p, p, p, 1, 77, 10, 16, 16, None) == -1
        assert _lib.last_error(htx).startswith("gl_set_conditioning_ti:") and "grounding = 0 (text)" in _lib.last_error(htx)
        # the shape rule of gl_set_conditioning_hw, on the right handle, still before anything is read
        assert l.gl_set_conditioning_ti(hti, p, p, p, p, p, p, p, p, 1, 77, 10, 16, 20, None) == -1
        assert "h = 16, w = 20 must be positive multiples of 8" in _lib.last_error(hti)
        # a short buffer gets a truncated, terminated copy and the full length
        small = ctypes.create_string_buffer(8)
        assert l.gl_last_error(hti, small, 8) > 8 and small.value == b"gl_set_"
        assert l.gl_set_conditioning_ti(None, p, p, p, p, p, p, p, p, 1, 77, 10, 16, 16, None) == -1
    finally:
        l.gl_destroy(hti)
        l.gl_destroy(htx)


# ------------------------------------------------------------------------------------------- grounding tokenizer input
def test_text_image_grounding_net_input_round_trip():
    g = TextImageGroundingNetInput()
    with pytest.raises(AssertionError):
        g.get_null_input()
    batch = {k: T(v) for k, v in tc.case_inputs(tc.by_name("ti_posnet")).items()}
    batch["unrelated"] = torch.zeros(1)
    out = g.prepare(batch)                              # the reference's one-argument call
    assert tuple(out) == TextImageGroundingNetInput.KEYS == ti_ref.KEYS and all(out[k] is batch[k] for k in out)
    assert g.prepare(batch, None).keys() == out.keys()  # ... and interface.py:516's two-argument call
    assert (g.batch, g.max_box, g.in_dim) == (2, 30, 768)
    null = g.get_null_input()
    assert {k: tuple(v.shape) for k, v in null.items()} == {k: tuple(v.shape) for k, v in out.items()}
    assert all(float(v.abs().max()) == 0.0 and v.dtype == torch.float32 for v in null.values())
    assert tuple(g.get_null_input(batch=3)["image_embeddings"].shape) == (3, 30, 768)
    assert isinstance(grounding_input_for(tc.TI_TINY), TextImageGroundingNetInput)
    assert type(grounding_input_for(TINY)) is GroundingNetInput


# ------------------------------------------------------------------------------------------- prepare_batch with images
class _StubClip:
    """``get_image_features`` of a CLIPModel: a fixed linear map of the mean pixel rows, so distinct images give distinct features"""

    def __init__(self, dim=768):
        self.calls = 0
        self.w = T(recipe.normal("stub.clip.w", (3 * 8, dim), 3))

    def get_image_features(self, pixel_values=None):
        self.calls += 1
        px = pixel_values.float()
        return px.reshape(px.shape[0], 3, 8, -1).mean(-1).reshape(px.shape[0], -1) @ self.w


class _StubProcessor:
    def __init__(self):
        self.image_calls = 0

    def __call__(self, text=None, images=None, return_tensors="pt", padding=True):
        if images is not None:
            self.image_calls += 1
            assert all(im.mode == "RGB" for im in images)
            arr = np.stack([np.asarray(im.resize((16, 16)), np.float32).transpose(2, 0, 1) / 255.0 for im in images])
            return {"pixel_values": T(arr)}
        raise AssertionError("no phrase is encoded in these tests")


def _png(path, seed, mode="RGB"):
    from PIL import Image
    a = (np.abs(recipe.uniform(f"ti.img.{seed}", (20, 28, 3), 5)) * 255).astype(np.uint8)
    im = Image.fromarray(a)
    if mode != "RGB":
        im = im.convert(mode)
    im.save(path)
    return str(path)


@pytest.fixture()
def torch_feature(monkeypatch):
    """the device op of the image branch replaced by the torch expression of interface.py:126-129 (the kernel itself: tests/test_gpu_ti.py)"""
    from layoutllm_t2i_amd import ops
    monkeypatch.setattr(ops, "image_ground_feature", lambda f, P, norm=28.7, out=None: (f @ P) / (f @ P).norm(dim=-1, keepdim=True) * norm)
    itf._PROJECTION_CACHE.clear()


def test_prepare_batch_with_images(tmp_path, torch_feature, monkeypatch):
    from PIL import Image
    clip, proc = _StubClip(), _StubProcessor()
    P = T(recipe.normal("ti.P", (768, 768), 9)) / 28.0
    a, b = _png(tmp_path / "a.png", 1), _png(tmp_path / "b.png", 2, mode="L")        # a grey file: .convert("RGB") applies
    pil = Image.open(a)
    locs = [[0.1, 0.1, 0.5, 0.5], [0.2, 0.3, 0.9, 0.8], [0.0, 0.0, 1.0, 1.0], [0.3, 0.3, 0.6, 0.6]]
    meta = dict(phrases=None, images=[a, None, b, a], locations=locs, projection_matrix=P, image_mask=[1, 1, 1, 0])
    out = itf.prepare_batch(meta, clip, proc, batch=2, device="cpu")
    assert clip.calls == 2 and proc.image_calls == 2                                   # a.png is encoded once
    assert out["masks"][0].tolist() == [1.0] * 4 + [0.0] * 26
    assert out["image_masks"][1].tolist() == [1.0, 0.0, 1.0, 0.0] + [0.0] * 26         # None entry; meta["image_mask"] clears box 3
    assert float(out["text_masks"].abs().max()) == 0.0 and float(out["text_embeddings"].abs().max()) == 0.0
    ie = out["image_embeddings"]
    assert tuple(ie.shape) == (2, 30, 768) and torch.equal(ie[0], ie[1]) and torch.equal(ie[0, 0], ie[0, 3])
    assert float(ie[0, 1].abs().max()) == 0.0 and float(ie[0, 4:].abs().max()) == 0.0 and not torch.equal(ie[0, 0], ie[0, 2])
    np.testing.assert_allclose(ie[0, [0, 2]].norm(dim=-1).numpy(), 28.7, rtol=1e-5)
    want = itf.get_clip_feature(clip, proc, pil, "cpu", is_image=True, projection_matrix=P)     # a PIL.Image works like its path
    assert torch.equal(want[0], ie[0, 0])
    # per-prompt lists; a prompt without images; one image shared by two prompts is encoded once for the batch
    clip.calls = 0
    metam = dict(phrases=None, images=[[a, b], None, [None, a]], locations=[locs[:2], locs[:1], locs[:2]], projection_matrix=P)
    outm = itf.prepare_batch_multiple(metam, clip, proc, batch=3, device="cpu")
    assert clip.calls == 2
    assert outm["image_masks"][:, :2].tolist() == [[1.0, 1.0], [0.0, 0.0], [0.0, 1.0]] and outm["masks"].sum(-1).tolist() == [2.0, 1.0, 2.0]
    assert torch.equal(outm["image_embeddings"][0, 0], outm["image_embeddings"][2, 1]) and torch.equal(outm["image_embeddings"][0, 0], ie[0, 0])
    with pytest.raises(ValueError, match="one entry"):
        itf.prepare_batch(dict(phrases=None, images=[a], locations=locs, projection_matrix=P), clip, proc, device="cpu")


def test_projection_matrix_lookup(tmp_path, torch_feature, monkeypatch):
    clip, proc = _StubClip(), _StubProcessor()
    a = _png(tmp_path / "a.png", 1)
    meta = dict(phrases=None, images=[a], locations=[[0.1, 0.1, 0.5, 0.5]])
    monkeypatch.delenv("GLIGEN_PROJECTION_MATRIX", raising=False)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError) as ei:
        itf.prepare_batch(meta, clip, proc, device="cpu")
    msg = str(ei.value)
    assert "meta['projection_matrix']" in msg and "$GLIGEN_PROJECTION_MATRIX" in msg and os.path.join(str(tmp_path), "projection_matrix") in msg
    # no image, no lookup: a text-only meta never needs the matrix
    assert float(itf.prepare_batch(dict(phrases=None, images=[None], locations=meta["locations"]), clip, proc, device="cpu")["image_masks"].sum()) == 0
    P1, P2, P3 = (T(recipe.normal(f"ti.P{i}", (768, 768), 9)) for i in range(3))
    torch.save(P3, str(tmp_path / "projection_matrix"))          # 3. the working directory, where the reference reads it
    f3 = itf.prepare_batch(meta, clip, proc, device="cpu")["image_embeddings"][0, 0]
    torch.save(P2, str(tmp_path / "env.pt"))
    monkeypatch.setenv("GLIGEN_PROJECTION_MATRIX", str(tmp_path / "env.pt"))            # 2. the environment variable
    f2 = itf.prepare_batch(meta, clip, proc, device="cpu")["image_embeddings"][0, 0]
    torch.save(P1, str(tmp_path / "meta.pt"))
    f1 = itf.prepare_batch({**meta, "projection_matrix": str(tmp_path / "meta.pt")}, clip, proc, device="cpu")["image_embeddings"][0, 0]
    f1t = itf.prepare_batch({**meta, "projection_matrix": P1}, clip, proc, device="cpu")["image_embeddings"][0, 0]
    feat = lambda P: itf.get_clip_feature(clip, proc, a, "cpu", is_image=True, projection_matrix=P)[0]
    assert torch.equal(f1, feat(P1)) and torch.equal(f1t, f1) and torch.equal(f2, feat(P2)) and torch.equal(f3, feat(P3))
    assert not torch.equal(f1, f2) and not torch.equal(f2, f3)
    # loaded once: the cached matrix survives the file
    os.remove(str(tmp_path / "env.pt"))
    torch.save(P1, str(tmp_path / "env.pt"))
    assert torch.equal(itf.prepare_batch(meta, clip, proc, device="cpu")["image_embeddings"][0, 0], f2)


def test_images_on_a_text_only_checkpoint_raise():
    """_run refuses before any encoder runs (the reference would prepare image tokens and drop them)"""
    class _M:
        cfg = TINY
    am = (_M(), None, None, None, {})
    with pytest.raises(ValueError, match="text-only checkpoint"):
        itf.run_one_image(am, dict(batch_size=1), dict(prompt="x", phrases=["a"], images=["a.png"], locations=[[0, 0, 1, 1]]), None)
    with pytest.raises(ValueError, match="text-only checkpoint"):
        itf.run_batch_images(am, dict(batch_size=1), dict(prompts=["x"], phrases=[["a"]], images=[[None, "a.png"]], locations=[[[0, 0, 1, 1]]]), None)


# ------------------------------------------------------------------------------------------- tests/ti_ref.py vs the reference
_SD = None


def ti_sd():
    global _SD
    if _SD is None:
        _SD = {k: T(np.asarray(v)) for k, v in recipe.state_dict(tc.TI_TINY, 0).items()}
    return _SD


@pytest.mark.parametrize("case", tc.CASES, ids=[c["name"] for c in tc.CASES])
def test_ti_ref_matches_reference(case):
    """the tolerance of tests/test_oracle_golden.py::test_oracle_matches_reference, which pins the text twins"""
    inp = {a: T(v) for a, v in tc.case_inputs(case).items()}
    with torch.no_grad():
        if case["kind"] == "position_net":
            out = ti_ref.position_net(ti_sd(), *(inp[k] for k in ti_ref.KEYS), 8)
        else:
            fc = {a: T(v) for a, v in recipe.sd_first_conv(tc.TI_TINY, 0).items()} if case["sdconv"] else None
            out = ti_ref.unet_forward(ti_sd(), tc.TI_TINY, inp["x"], torch.tensor(case["t"]), inp["context"], inp["relations"], inp,
                                      fuser_scale=case["scale"], first_conv=fc)
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    assert out.shape == ref.shape
    scale = max(1.0, float(np.nanmax(np.abs(ref))))
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-4, atol=3e-5 * scale, equal_nan=True)


def test_goldens_see_every_grounding_input():
    """the fixtures can tell the masks apart: ti_ref with the image masks (or the text masks) zeroed is far from the reference's output"""
    case = tc.by_name("ti_posnet")
    inp = {a: T(v) for a, v in tc.case_inputs(case).items()}
    ref = np.load(os.path.join(GOLD, "ti_posnet.npz"))["out"]
    for k in ("text_masks", "image_masks", "masks"):
        out = ti_ref.position_net(ti_sd(), *((torch.zeros_like(inp[a]) if a == k else inp[a]) for a in ti_ref.KEYS), 8).numpy()
        assert np.abs(out - ref).max() > 1e-2, k
    null = np.load(os.path.join(GOLD, "ti_posnet_null.npz"))["out"]
    assert np.abs(null[:, :30] - null[:, :1]).max() == 0 and np.abs(null[:, 30:] - null[:, 30:31]).max() == 0      # MLP(null features) on every row
    assert np.abs(null[:, 0] - null[:, 30]).max() > 1e-2                                                             # ... one per chain
