"""CPU tests (no GPU) of the keypoint grounding family (``checkpoint_generation_keypoint.pth``): config parsing, parameter names against the
reference's, the engine's weight table against the packer (padded K of linears.0), the other families' tables byte for byte, gl_create's
refusals, the family check of the conditioning entries, the grounding-tokenizer input, prepare_batch_kp against the reference's own batch,
the interface's refusals, and tests/kp_ref.py against the reference's own outputs (tests/golden/kp_*.npz)."""
import ctypes
import dataclasses
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import kp_cases as kc
import kp_ref
from layoutllm_t2i_amd import _lib, arch, recipe, weights
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY, UNetConfig
from layoutllm_t2i_amd.model import GroundingNetInput, KeypointGroundingNetInput, UNetModel, grounding_input_for

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
PN_NAMES = ["position_net.person_emb", "position_net.keypoint_emb", "position_net.null_person", "position_net.null_xy"] + [
    f"position_net.linears.{i}.{s}" for i in (0, 2, 4) for s in ("w", "b")]


def _ensure_built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)


def _params(P=8, **kw):
    return {"model_channels": 64, "num_heads": 4, **kw,
            "grounding_tokenizer": {"target": kc.KP_TARGET, "params": {"max_persons_per_image": P, "out_dim": 768}}}


# ------------------------------------------------------------------------------------------- configuration
def test_from_dict_needs_the_flag():
    with pytest.raises(NotImplementedError, match="keypoint"):
        UNetConfig.from_dict(_params())
    with pytest.raises(NotImplementedError, match="allow_keypoint"):
        UNetConfig.from_dict(_params(), allow_inpaint=True)
    cfg = UNetConfig.from_dict(_params(), allow_keypoint=True)
    assert cfg.grounding == "keypoint" and cfg.max_persons == 8 and cfg.max_objs == 136 and cfg.n_ground == 136
    assert cfg.pos_in_dim == cfg.pos_out_dim == 768 and cfg.position_dim == 32 and cfg.relation is False
    assert dataclasses.replace(cfg, image_size=16) == kc.KP_TINY[8]
    # the box families keep their Fourier width and have no persons
    assert TINY.position_dim == 64
    with pytest.raises(AttributeError, match="persons"):
        TINY.max_persons


@pytest.mark.parametrize("P,ok", [(0, False), (1, True), (3, True), (8, True), (9, False), (-1, False)])
def test_person_bounds(P, ok):
    if ok:
        cfg = UNetConfig.from_dict(_params(P), allow_keypoint=True)
        assert cfg.max_persons == P and cfg.max_objs == 17 * P
    else:
        with pytest.raises(ValueError, match="max_persons_per_image"):
            UNetConfig.from_dict(_params(P), allow_keypoint=True)


def test_keypoint_with_inpaint_mode_is_refused():
    with pytest.raises(NotImplementedError, match="inpaint_mode"):
        UNetConfig.from_dict(_params(inpaint_mode=True), allow_inpaint=True, allow_keypoint=True)


def test_param_shapes_equal_the_reference_models():
    """names, order and shapes of the reference model's own state dict (tools/make_kp_goldens.py, kp_params)"""
    z = np.load(os.path.join(GOLD, "kp_params.npz"))
    want = [(str(n), tuple(int(v) for v in str(s).split(",")) if str(s) else ()) for n, s in zip(z["names"], z["shapes"])]
    got = list(arch.param_shapes(kc.KP_TINY[3]).items())
    assert got == want
    pn = dict(got)
    assert pn["position_net.person_embeddings"] == (3, 768) and pn["position_net.keypoint_embeddings"] == (17, 768)
    assert pn["position_net.linears.0.weight"] == (512, 800) and pn["position_net.null_xy_feature"] == (32,)
    assert [k for k, _ in got if k.startswith("position_net.")][:5] == [
        "position_net.person_embeddings", "position_net.keypoint_embeddings", "position_net.null_person_feature", "position_net.null_xy_feature",
        "position_net.linears.0.weight"]
    assert not any(".rela_fuse." in k for k, _ in got)


# ------------------------------------------------------------------------------------------- weight table
@pytest.mark.parametrize("split", [False, True], ids=["compact", "split"])
def test_weight_table_equals_the_packer(split):
    _ensure_built()
    cfg = dataclasses.replace(kc.KP_TINY[3], split_weights=split)
    text = dataclasses.replace(TINY, relation=False, split_weights=split)
    h, ht = _lib.create_engine(cfg), _lib.create_engine(text)
    try:
        table, total = _lib.weight_table(h)
        text_table, _ = _lib.weight_table(ht)
    finally:
        _lib.lib().gl_destroy(h)
        _lib.lib().gl_destroy(ht)
    names = [t[0] for t in table]
    assert [n for n in names if n.startswith("position_net.")] == PN_NAMES
    body = lambda tb: [(t[0], t[1], t[2], t[3], t[4]) for t in tb if not t[0].startswith("position_net.")]
    assert body(table) == body(text_table)                     # every other name, offset and shape is the text table's
    shapes, dtypes = {t[0]: t[4] for t in table}, {t[0]: t[3] for t in table}
    k = 2 if split else 1
    assert shapes["position_net.linears.0.w"] == (512, 832 * k) and shapes["position_net.linears.2.w"] == (512, 512 * k)
    assert shapes["position_net.linears.4.w"] == (768, 512 * k)
    assert shapes["position_net.person_emb"] == (3, 768) and shapes["position_net.keypoint_emb"] == (17, 768)
    assert shapes["position_net.null_person"] == (768,) and shapes["position_net.null_xy"] == (32,)
    assert all(dtypes[n] == 1 for n in PN_NAMES[:4])            # the tables and the null features stay fp32
    sd = recipe.state_dict(cfg, 0)
    P = weights.pack_state_dict(sd, cfg, "cpu")
    assert P.flat.numel() == total and set(P.w) == set(names)
    for name, off, nbytes, dtype, shape in table:
        assert tuple(P.w[name].shape) == tuple(shape) and P.w[name].data_ptr() == P.flat.data_ptr() + off
    # linears.0: the checkpoint's 800 columns, then zeros up to 832 -- in a split table each of the [Whi | Wlo] halves on its own
    w = T(sd["position_net.linears.0.weight"])
    pw = P.w["position_net.linears.0.w"]
    assert torch.equal(pw[:, :800], w.half()) and float(pw[:, 800:832].abs().max()) == 0.0
    if split:
        assert torch.equal(pw[:, 832:1632], (w - w.half().float()).half()) and float(pw[:, 1632:].abs().max()) == 0.0
        assert float(pw[:, 832:1632].abs().max()) > 0.0
    assert torch.equal(P.w["position_net.person_emb"], T(sd["position_net.person_embeddings"]))
    assert torch.equal(P.w["position_net.keypoint_emb"], T(sd["position_net.keypoint_embeddings"]))
    assert torch.equal(P.w["position_net.null_person"], T(sd["position_net.null_person_feature"]))
    assert torch.equal(P.w["position_net.null_xy"], T(sd["position_net.null_xy_feature"]))
    with pytest.raises(KeyError, match="missing"):
        weights.pack_state_dict(recipe.state_dict(text, 0), cfg, "cpu")


# sha256 of pack_state_dict(recipe.state_dict(cfg, 0), cfg, "cpu", recipe.sd_first_conv(cfg, 0)).flat on the commit BEFORE the keypoint family
# (TINY with the named grounding and split_weights): the text and text_image tables keep their bytes
PARENT_DIGESTS = {
    ("text", False): (122945792, "e0c59fbdf6bd80a9eb1072c4387984c424671603ea93a645ea85fef72da56302"),
    ("text", True): (237368064, "511d1ba0b8182345886df348e48e94964d2e5869bbb46b6359291af9263a1106"),
    ("text_image", False): (125118720, "7eaffb72692f355e4e4614b96bd0a13c1ef8856fe14ebb4d8005e5997195af86"),
    ("text_image", True): (241703680, "5aa483793f3bf0ac9c66ba42a754faedf2d3de20e921574d7611ec2902114a0a"),
}


@pytest.mark.parametrize("grounding,split", list(PARENT_DIGESTS), ids=[f"{g}-{'split' if s else 'compact'}" for g, s in PARENT_DIGESTS])
def test_other_families_tables_keep_their_bytes(grounding, split):
    _ensure_built()
    cfg = dataclasses.replace(TINY, grounding=grounding, split_weights=split)
    P = weights.pack_state_dict(recipe.state_dict(cfg, 0), cfg, "cpu", recipe.sd_first_conv(cfg, 0))
    assert (P.flat.numel(), hashlib.sha256(P.flat.numpy().tobytes()).hexdigest()) == PARENT_DIGESTS[(grounding, split)]


def test_abi_is_additive():
    _ensure_built()
    assert _lib.ABI_VERSION == 15 and _lib.lib().gl_abi_version() == 15
    assert ctypes.sizeof(_lib.UNetConfigC) == _lib.lib().gl_sizeof_unet_config()
    assert _lib.unet_config_c(kc.KP_TINY[8]).grounding == 2 and _lib.unet_config_c(kc.KP_TINY[8]).no_relation == 1
    assert _lib.unet_config_c(TINY).grounding == 0


# ------------------------------------------------------------------------------------------- gl_create
def _create_rc(cfg, **fields):
    l = _lib.lib()
    cc, h = _lib.unet_config_c(cfg), ctypes.c_void_p()
    for k, v in fields.items():
        setattr(cc, k, v)
    rc = l.gl_create(ctypes.byref(cc), ctypes.byref(h))
    if rc == 0:
        l.gl_destroy(h)
    return rc


def test_gl_create_refusals():
    """GL_ERR_UNSUPPORTED (-2): the relation block, inpaint_mode, a token count that is no multiple of 17, more than 8 persons; the box
    families keep their 64-token limit"""
    _ensure_built()
    kp = kc.KP_TINY[8]
    assert _create_rc(kp) == 0 and _create_rc(kc.KP_TINY[1]) == 0 and _create_rc(kc.KP_TINY[3]) == 0
    assert _create_rc(kp, no_relation=0) == -2
    assert _create_rc(kp, inpaint_mode=1) == -2
    assert _create_rc(kp, max_objs=18) == -2
    assert _create_rc(kp, max_objs=153) == -2
    assert _create_rc(kp, max_objs=0) == -2
    assert _create_rc(kp, pos_in_dim=512) == -2                 # the person features are as wide as the tokens
    assert _create_rc(kp, grounding=3) == -2
    assert _create_rc(dataclasses.replace(TINY, max_objs=64)) == 0 and _create_rc(dataclasses.replace(TINY, max_objs=65)) == -2
    assert _create_rc(dataclasses.replace(TINY, max_objs=68, relation=False)) == -2       # 4 x 17 tokens, but a text handle


def test_conditioning_entries_check_the_family():
    """every conditioning entry on a handle of another family returns GL_ERR_BAD_ARG (-1) with a message that names the right entry, before
    it reads any argument: no GPU, no weights, dummy pointers"""
    _ensure_built()
    l = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    ti = dataclasses.replace(TINY, grounding="text_image")
    hk, hx, hi = _lib.create_engine(kc.KP_TINY[3]), _lib.create_engine(TINY), _lib.create_engine(ti)
    try:
        assert l.gl_set_conditioning(hk, p, p, p, p, p, 1, 77, 10, 16, None) == -1
        e = _lib.last_error(hk)
        assert e.startswith("gl_set_conditioning:") and "grounding = 2 (keypoint)" in e and e.endswith("use gl_set_conditioning_kp")
        assert l.gl_set_conditioning_hw(hk, p, p, p, p, p, 1, 77, 10, 16, 24, None) == -1
        assert _lib.last_error(hk).startswith("gl_set_conditioning_hw:") and "gl_set_conditioning_kp" in _lib.last_error(hk)
        assert l.gl_set_conditioning_ti(hk, p, p, p, p, p, p, p, p, 1, 77, 10, 16, 16, None) == -1
        assert _lib.last_error(hk).startswith("gl_set_conditioning_ti:") and "gl_set_conditioning_kp" in _lib.last_error(hk)
        assert l.gl_set_conditioning_kp(hx, p, p, p, 1, 77, 16, 16, None) == -1
        e = _lib.last_error(hx)
        assert e.startswith("gl_set_conditioning_kp:") and "grounding = 0 (text)" in e and "gl_set_conditioning / gl_set_conditioning_hw" in e
        assert l.gl_set_conditioning_kp(hi, p, p, p, 1, 77, 16, 16, None) == -1
        e = _lib.last_error(hi)
        assert e.startswith("gl_set_conditioning_kp:") and "grounding = 1 (text_image)" in e and e.endswith("use gl_set_conditioning_ti")
        # the shape rule of gl_set_conditioning_hw, on the right handle, still before anything is read
        assert l.gl_set_conditioning_kp(hk, p, p, p, 1, 77, 16, 20, None) == -1
        assert "h = 16, w = 20 must be positive multiples of 8" in _lib.last_error(hk)
        # the right family and a legal shape, but no weights loaded: refused without touching a pointer
        assert l.gl_set_conditioning_kp(hk, p, p, p, 1, 77, 16, 16, None) == -1
        assert l.gl_set_conditioning_kp(None, p, p, p, 1, 77, 16, 16, None) == -1
    finally:
        for h in (hk, hx, hi):
            l.gl_destroy(h)


# ------------------------------------------------------------------------------------------- grounding tokenizer input, model dispatch
def test_keypoint_grounding_net_input_round_trip():
    g = KeypointGroundingNetInput()
    with pytest.raises(AssertionError):
        g.get_null_input()
    batch = {k: T(v) for k, v in kc.case_inputs(kc.by_name("kp_posnet_p3")).items()}
    out = g.prepare(batch)                              # the reference's one-argument call
    assert tuple(out) == KeypointGroundingNetInput.KEYS == kp_ref.KEYS and all(out[k] is batch[k] for k in out)
    assert g.prepare(batch, None).keys() == out.keys()  # ... and interface.py:516's two-argument call
    assert (g.batch, g.max_persons_per_image) == (2, 3)
    null = g.get_null_input()
    assert {k: tuple(v.shape) for k, v in null.items()} == {"points": (2, 51, 2), "masks": (2, 51)}
    assert all(float(v.abs().max()) == 0.0 and v.dtype == torch.float32 for v in null.values())
    assert tuple(g.get_null_input(batch=3)["points"].shape) == (3, 51, 2)
    assert isinstance(grounding_input_for(kc.KP_TINY[3]), KeypointGroundingNetInput)
    assert type(grounding_input_for(TINY)) is GroundingNetInput


class _Engine:
    def __init__(self):
        self.calls = []

    def set_conditioning_kp(self, context, points, masks, hw):
        self.calls.append(("kp", tuple(points.shape), tuple(masks.shape), hw))

    def set_conditioning(self, *a, **k):
        raise AssertionError("the box entry on a keypoint model")


def test_model_dispatches_on_the_family():
    m = UNetModel.from_packed(None, kc.KP_TINY[3], "cpu")
    m.engine, m.grounding_tokenizer_input = _Engine(), None
    pts, msk = torch.zeros(2, 51, 2), torch.zeros(2, 51)
    m.set_conditioning(torch.zeros(2, 77, 768), None, {"points": pts, "masks": msk}, (16, 24))
    assert m.engine.calls == [("kp", (2, 51, 2), (2, 51), (16, 24))]
    with pytest.raises(ValueError, match=r"missing \['points'\]"):
        m.set_conditioning(torch.zeros(2, 77, 768), None, {"masks": msk}, 16)
    with pytest.raises(ValueError, match="points"):
        m.set_conditioning(torch.zeros(2, 77, 768), None, {"boxes": pts, "masks": msk, "positive_embeddings": pts}, 16)
    with pytest.raises(RuntimeError, match="grounding_tokenizer_input"):
        m.grounding_of({})
    m.grounding_tokenizer_input = grounding_input_for(m.cfg)
    m.grounding_tokenizer_input.prepare({"points": pts, "masks": msk})
    assert set(m.grounding_of({})) == {"points", "masks"}


# ------------------------------------------------------------------------------------------- prepare_batch_kp, the interface
def _ref_batch():
    z = np.load(os.path.join(GOLD, "kp_prepare_batch.npz"))
    return z["locations"].tolist(), z["points"], z["masks"]


def test_prepare_batch_kp_matches_the_reference():
    locations, points, masks = _ref_batch()
    assert len(locations) == 2 and all(len(p) == 17 for p in locations)
    out = itf.prepare_batch_kp(dict(locations=locations), batch=2, max_persons=8, device="cpu")
    assert tuple(out) == ("points", "masks") and out["points"].dtype == torch.float32 and out["masks"].dtype == torch.float32
    np.testing.assert_array_equal(out["points"].numpy(), points)
    np.testing.assert_array_equal(out["masks"].numpy(), masks)
    assert float(out["masks"][0].sum()) == 19.0 and float(out["masks"][0, 34:].abs().max()) == 0.0      # 11 + 8 visible keypoints, persons 2..7 absent
    out3 = itf.prepare_batch_kp(dict(locations=locations), batch=1, max_persons=3)
    assert tuple(out3["points"].shape) == (1, 51, 2) and torch.equal(out3["points"][0, :34], out["points"][0, :34])
    multi = itf.prepare_batch_kp_multiple(dict(locations=[locations, locations[:1]]), 2, 8, "cpu")
    assert torch.equal(multi["points"][0], out["points"][0]) and torch.equal(multi["points"][1, :17], out["points"][0, :17])
    assert float(multi["masks"][1, 17:].abs().max()) == 0.0


def test_prepare_batch_kp_refusals():
    locations, _, _ = _ref_batch()
    with pytest.raises(ValueError, match="3 persons"):
        itf.prepare_batch_kp(dict(locations=[locations[0]] * 3), max_persons=2)
    with pytest.raises(ValueError, match="person 1 has 16 keypoints"):
        itf.prepare_batch_kp(dict(locations=[locations[0], locations[1][:16]]))
    with pytest.raises(ValueError, match="pose layouts"):
        itf.prepare_batch_kp_multiple(dict(locations=[locations]), 2)


def test_interface_refusals_on_a_keypoint_model():
    """_run refuses before any encoder runs"""
    class _M:
        cfg = kc.KP_TINY[8]
    am = (_M(), None, None, None, {})
    locations, _, _ = _ref_batch()
    with pytest.raises(ValueError, match=r"meta\['images'\]"):
        itf.run_one_image(am, dict(batch_size=1), dict(prompt="x", images=["a.png"], locations=locations), None)
    with pytest.raises(ValueError, match=r"meta\['input_image'\]"):
        itf.run_one_image(am, dict(batch_size=1), dict(prompt="x", input_image="a.png", locations=locations), None)
    with pytest.raises(ValueError, match=r"meta\['input_image'\]"):
        itf.run_batch_images(am, dict(batch_size=1), dict(prompts=["x"], input_image=["a.png"], locations=[locations]), None)


def test_load_ckpt_refuses_relation_tensors_and_the_sharded_entry(tmp_path, monkeypatch):
    cfg = kc.KP_TINY[1]
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    rela = next(k for k in arch.param_shapes(TINY) if ".rela_fuse." in k)
    config = {"model": {"params": dict(image_size=16, model_channels=64, num_heads=4,
                                       grounding_tokenizer={"target": kc.KP_TARGET, "params": {"max_persons_per_image": 1, "out_dim": 768}})}}
    path = str(tmp_path / "kp.pth")
    torch.save({"model": {**sd, rela: torch.zeros(1)}, "config_dict": {"_content": config}}, path)
    with pytest.raises(NotImplementedError, match="rela_fuse"):
        itf.load_ckpt(path, "cpu")

    class _M:
        pass
    m = _M()
    m.cfg = cfg
    monkeypatch.setattr(itf, "load_all_models", lambda *a, **k: (m, None, None, None, {}))
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda *a, **k: 0)
    with pytest.raises(NotImplementedError, match="keypoint checkpoint"):
        itf.load_all_models_sharded(path, "cpu")


# ------------------------------------------------------------------------------------------- tests/kp_ref.py vs the reference
_SD = {}


def kp_sd(cfg):
    if cfg not in _SD:
        _SD[cfg] = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    return _SD[cfg]


@pytest.mark.parametrize("case", kc.POSNET_CASES + kc.UNET_CASES, ids=[c["name"] for c in kc.POSNET_CASES + kc.UNET_CASES])
def test_kp_ref_matches_reference(case):
    """fp32 against the reference's own fp32 output: rtol 1e-5 / atol 1e-6"""
    cfg = kc.cfg_of(case)
    inp = {a: T(v) for a, v in kc.case_inputs(case).items()}
    with torch.no_grad():
        if case["kind"] == "position_net":
            sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="position_net.").items()}
            out = kp_ref.position_net(sd, inp["points"], inp["masks"], 8)
        else:
            fc = {a: T(v) for a, v in recipe.sd_first_conv(cfg, 0).items()} if case["sdconv"] else None
            g = {k: inp[k] for k in kp_ref.KEYS}
            if case["grounding"] == "null":
                g = kp_ref.null_grounding(g)
            out = kp_ref.unet_forward(kp_sd(cfg), cfg, inp["x"], torch.tensor(case["t"]), inp["context"], g, fuser_scale=case["scale"], first_conv=fc)
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    assert out.shape == ref.shape
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-5, atol=1e-6)


def test_goldens_see_the_grounding_inputs():
    """the fixtures can tell persons, keypoints, points and masks apart"""
    case = kc.by_name("kp_posnet_p3")
    cfg = kc.cfg_of(case)
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="position_net.").items()}
    inp = {a: T(v) for a, v in kc.case_inputs(case).items()}
    ref = np.load(os.path.join(GOLD, "kp_posnet_p3.npz"))["out"]
    m = inp["masks"]
    assert 0.0 < float(m[0, 0]) < 1.0 and float(m[:, 34:].abs().max()) == 0.0 and 0 < int((m[:, :34] == 0).sum()) < 34      # fractional, absent person, missing keypoints
    assert np.abs(kp_ref.position_net(sd, inp["points"], torch.zeros_like(m), 8).numpy() - ref).max() > 1e-2
    assert np.abs(kp_ref.position_net(sd, torch.zeros_like(inp["points"]), m, 8).numpy() - ref).max() > 1e-2
    for k in ("position_net.person_embeddings", "position_net.keypoint_embeddings"):
        rolled = {**sd, k: torch.roll(sd[k], 1, 0)}
        assert np.abs(kp_ref.position_net(rolled, inp["points"], m, 8).numpy() - ref).max() > 1e-2, k
    assert np.abs(ref[:, 34:] - ref[:, 34:35]).max() == 0                # an absent person: MLP(null features) on every row
    # the UNet fixtures: real grounding differs from null grounding, scale 0 does not see the tokens at all
    real, null = (np.load(os.path.join(GOLD, n + ".npz"))["out"] for n in ("kp_unet_tiny_p8_s1", "kp_unet_tiny_null"))
    assert np.linalg.norm(real - null) / np.linalg.norm(null) > 1e-2
    s0 = [np.load(os.path.join(GOLD, f"kp_unet_tiny_p{P}_s0_sd.npz"))["out"] for P in (3, 8)]
    np.testing.assert_array_equal(s0[0], s0[1])
