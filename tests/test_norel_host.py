"""CPU tests (no GPU) of the UNet without the rela_fuse chain (``UNetConfig.relation = False``: the upstream GLIGEN transformer block that every
public GLIGEN checkpoint was trained on): tests/norel_ref.py against the reference's pre-modification UNet (tests/golden/norel_*.npz), the
engine's weight table and the packer, checkpoint detection in ``interface.load_ckpt``, the refusals, the negative prompt, and the FLOP count."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import norel_cases as nc
import norel_ref
import stubs
from layoutllm_t2i_amd import _lib, arch, flops, recipe, weights
from layoutllm_t2i_amd import gligen_inference as gi
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, UNetConfig
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.model import LatentDiffusion, UNetModel
from layoutllm_t2i_amd.sampler import PLMSSampler
from oracle import plms_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy


def _ensure_built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)


_SD = {}


def sd_of(cfg):
    if cfg not in _SD:
        _SD[cfg] = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items()}
    return _SD[cfg]


# ------------------------------------------------------------------------------------------- configuration and shapes
def test_relation_defaults_to_true_and_drops_only_rela_fuse():
    assert UNetConfig().relation is True and TINY.relation is True and nc.NR_TINY.relation is False
    assert UNetConfig.from_dict(dict(model_channels=64, num_heads=4)).relation is True         # not a key of the config dict
    for rel, nr in ((TINY, nc.NR_TINY), (dataclasses.replace(TINY, grounding="text_image"), nc.NR_TI_TINY),
                    (dataclasses.replace(TINY, inpaint_mode=True), nc.NR_IP_TINY)):
        a, b = arch.param_shapes(rel), arch.param_shapes(nr)
        assert [k for k in a if ".rela_fuse." not in k] == list(b) and all(a[k] == b[k] for k in b)
        assert len(a) - len(b) == 17 * len(arch.build_plan(rel).st_layers())
    assert len(arch.param_shapes(TINY)) == 1238 and len(arch.param_shapes(nc.NR_TINY)) == 966
    # recipe tensors are pure functions of their name: the other tensors are those of the relation-aware model
    full, part = recipe.state_dict(TINY, 0), recipe.state_dict(nc.NR_TINY, 0)
    assert set(full) - set(part) == {k for k in full if ".rela_fuse." in k}
    for k in ("input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight", "middle_block.1.transformer_blocks.0.fuser.alpha_attn", "out.2.bias"):
        assert np.array_equal(full[k], part[k])
    rs = weights.random_state_dict(nc.NR_TINY, "cpu")
    assert list(rs) == list(part)


def test_flops_drop_exactly_the_rela_fuse_terms():
    lin = lambda m, k, n: 2.0 * m * k * n
    for cfg in (TINY, UNetConfig()):
        for hw in (16, (8, 16), 64):
            for fuser_on in (True, False):
                want = 0.0
                for l in arch.build_plan(cfg).st_layers():
                    C, mo, ctx, R = l.cin, cfg.max_objs, cfg.context_dim, 10
                    want += lin(mo, C, C) + 2 * lin(R, ctx, C) + 2.0 * 2.0 * mo * R * C + lin(mo, C, C)      # q, k / v, QK^T + PV, to_out
                    want += lin(mo, C, 8 * C) + lin(mo, 4 * C, C)                                            # the GEGLU feed-forward
                got = flops.unet_forward_flops(cfg, hw, fuser_on) - flops.unet_forward_flops(dataclasses.replace(cfg, relation=False), hw, fuser_on)
                assert got == pytest.approx(want, rel=1e-9) and want > 0
    assert flops.unet_forward_flops(UNetConfig(), 64) == pytest.approx(1.1477e12, rel=1e-3)      # the relation figure is unchanged


# ------------------------------------------------------------------------------------------- tests/norel_ref.py vs the reference
@pytest.mark.parametrize("case", nc.UNET_CASES, ids=[c["name"] for c in nc.UNET_CASES])
def test_norel_ref_matches_reference(case):
    """the tolerance of tests/test_oracle_golden.py::test_oracle_matches_reference, which pins unet_tiny_*"""
    cfg = nc.cfg_of(case)
    inp = {a: T(v) for a, v in nc.case_inputs(case).items()}
    g = {k: inp[k] for k in nc.grounding_keys(cfg)}
    null = case["grounding"] == "null"
    fc = {a: T(v) for a, v in recipe.sd_first_conv(cfg, 0).items()} if case["sdconv"] else None
    sd = sd_of(cfg)
    assert not any("rela_fuse" in k for k in sd)
    with torch.no_grad():
        out = norel_ref.unet_forward(sd, cfg, inp["x"], torch.tensor(case["t"]), inp["uc"] if null else inp["context"],
                                     norel_ref.null_grounding(g) if null else g, fuser_scale=case["scale"], first_conv=fc, extra=inp.get("extra"))
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    assert out.shape == ref.shape
    scale = max(1.0, float(np.nanmax(np.abs(ref))))
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-4, atol=3e-5 * scale, equal_nan=True)


def test_norel_goldens_are_far_from_the_relation_goldens():
    """the sibling cases share inputs and every tensor but rela_fuse's: a parity test of the new path cannot be met by the relation path"""
    for a, b in (("norel_unet_tiny_cond", "unet_tiny_cond"), ("norel_unet_tiny_null", "unet_tiny_null"), ("norel_unet_tiny_s0_sd", "unet_tiny_s0_sd"),
                 ("norel_ti_unet_tiny_s1", "ti_unet_tiny_s1"), ("norel_ip9_unet_tiny_s1", "ip9_unet_tiny_s1"), ("norel_plms_tiny", "plms_tiny")):
        x, y = (np.load(os.path.join(GOLD, n + ".npz"))["out"] for n in (a, b))
        r = float(np.linalg.norm(x - y) / np.linalg.norm(x))
        assert r > 0.1, (a, b, r)


def test_norel_plms_tiny_matches_reference():
    """the bound of tests/test_oracle_golden.py::test_plms_tiny_matches_reference"""
    case = nc.by_name("norel_plms_tiny")
    inp = {a: T(v) for a, v in nc.case_inputs(case).items()}
    fc = {a: T(v) for a, v in recipe.sd_first_conv(nc.NR_TINY, 0).items()}
    with torch.no_grad():
        out = plms_ref.plms_sample(norel_ref.make_eps_fn(sd_of(nc.NR_TINY), nc.NR_TINY, inp, case["guidance"], fc), inp["x"], case["S"],
                                   case["alpha_type"])
    ref = np.load(os.path.join(GOLD, "norel_plms_tiny.npz"))["out"]
    err = np.abs(out.numpy() - ref).max() / np.abs(ref).max()
    assert err < 2e-4, err


# ------------------------------------------------------------------------------------------- the weight table and the packer
def _table(cfg):
    h = _lib.create_engine(cfg)
    try:
        return _lib.weight_table(h)
    finally:
        _lib.lib().gl_destroy(h)


def test_config_struct_keeps_abi_15_and_a_zeroed_field_is_todays_table():
    _ensure_built()
    l = _lib.lib()
    assert ctypes.sizeof(_lib.UNetConfigC) == l.gl_sizeof_unet_config() and l.gl_abi_version() == 15 == _lib.ABI_VERSION
    assert _lib.UNetConfigC._fields_[-1][0] == "no_relation"                       # the trailing field
    assert _lib.unet_config_c(TINY).no_relation == 0 and _lib.unet_config_c(nc.NR_TINY).no_relation == 1
    table, total = _table(TINY)
    # the table of the parent commit: 1102 entries, 256 of them rela_fuse's (16 per transformer), 122945792 bytes
    assert len(table) == 1102 and total == 122945792 and sum("rela_fuse" in t[0] for t in table) == 256
    cc, h = _lib.unet_config_c(nc.NR_TINY), ctypes.c_void_p()
    cc.no_relation = 0                                                              # zeroed by hand: the relation table again
    assert l.gl_create(ctypes.byref(cc), ctypes.byref(h)) == 0
    try:
        assert _lib.weight_table(h.value) == (table, total)
    finally:
        l.gl_destroy(h)
    cc.no_relation = 2
    assert l.gl_create(ctypes.byref(cc), ctypes.byref(h)) != 0


@pytest.mark.parametrize("family", ["text", "text_image", "inpaint"])
@pytest.mark.parametrize("split", [False, True], ids=["compact", "split"])
def test_weight_table_without_rela_fuse(family, split):
    """no name containing rela_fuse; every other entry has the name, dtype and shape of the relation table, in its order; the packer fills it"""
    _ensure_built()
    nr = dataclasses.replace({"text": nc.NR_TINY, "text_image": nc.NR_TI_TINY, "inpaint": nc.NR_IP_TINY}[family], split_weights=split)
    rel = dataclasses.replace(nr, relation=True)
    table, total = _table(nr)
    rtable, rtotal = _table(rel)
    assert not any("rela_fuse" in t[0] for t in table)
    strip = lambda tab: [(n, nb, dt, shp) for n, off, nb, dt, shp in tab if "rela_fuse" not in n]
    assert strip(table) == strip(rtable)
    pad = lambda nb: (nb + 255) // 256 * 256
    assert total == rtotal - sum(pad(t[2]) for t in rtable if "rela_fuse" in t[0]) and total == sum(pad(t[2]) for t in table)
    assert all(off % 256 == 0 for _, off, *_r in table)
    sd = recipe.state_dict(nr, 0)
    P = weights.pack_state_dict(sd, nr, "cpu", None if nr.inpaint_mode else recipe.sd_first_conv(nr, 0))
    assert P.flat.numel() == total and set(P.w) == {t[0] for t in table} and not any("rela_fuse" in k for k in P.s)
    # ... with the same bytes as the relation handle's packed tensors of the same name
    Pr = weights.pack_state_dict(recipe.state_dict(rel, 0), rel, "cpu", None if nr.inpaint_mode else recipe.sd_first_conv(nr, 0))
    assert all(torch.equal(P.w[k], Pr.w[k]) for k in P.w)
    assert all(P.s[k] == Pr.s[k] for k in P.s) and len(Pr.s) == 2 * len(P.s)
    # round trip through the flat buffer (what the sharded broadcast would carry)
    Q = weights.PackedWeights.from_flat(P.flat, nr, "cpu", P.has_sd_conv)
    assert set(Q.w) == set(P.w) and Q.s == P.s


def test_an_explicit_relation_config_still_needs_the_tensors():
    _ensure_built()
    sd = recipe.state_dict(nc.NR_TINY, 0)
    with pytest.raises(KeyError, match=r"missing 272 tensors.*rela_fuse"):
        weights.pack_state_dict(sd, TINY, "cpu")
    # the other way round: unexpected keys are ignored (strict=False semantics), the chain is simply not packed
    P = weights.pack_state_dict(recipe.state_dict(TINY, 0), nc.NR_TINY, "cpu")
    assert not any("rela_fuse" in k for k in P.w)


# ------------------------------------------------------------------------------------------- checkpoint detection
class _Any:
    device = "cpu"

    def to(self, d):
        return self

    def eval(self):
        return self

    def load_state_dict(self, sd):
        pass


class _FakeUNet:
    built = []

    def __init__(self, cfg, state_dict, device=None, sd_first_conv=None, allow_missing_sd_conv=False):
        self.cfg, self.sd, self.strict = cfg, state_dict, False
        _FakeUNet.built.append(self)

    def set_strict(self, on=True):
        self.strict = on
        return self


@pytest.fixture()
def no_engine(monkeypatch):
    """interface.load_ckpt with the engine, the VAE and the text encoder patched out: what is left is the config and the detection"""
    monkeypatch.setattr(itf, "UNetModel", _FakeUNet)
    monkeypatch.setattr(itf, "_instantiate_reference", lambda node: _Any())
    monkeypatch.setenv("GLIGEN_REFERENCE_VAE", "1")
    monkeypatch.setenv("GLIGEN_REFERENCE_TEXT_ENCODER", "1")
    _FakeUNet.built.clear()


def _checkpoint(path, drop=lambda k: False, inpaint=False):
    ck = stubs.write_synthetic_checkpoint(path, TINY, VAE_TINY)
    if inpaint:
        ck["config_dict"]["_content"]["model"]["params"]["inpaint_mode"] = True
    ck["model"] = {k: v for k, v in ck["model"].items() if not drop(k)}
    torch.save(ck, path)
    return ck


def test_load_ckpt_detects_the_block_from_the_state_dict(no_engine, tmp_path):
    p = str(tmp_path / "ck.pth")
    _checkpoint(p)
    model = itf.load_ckpt(p, "cpu")[0]
    assert model.cfg.relation is True and model.cfg == dataclasses.replace(TINY, image_size=model.cfg.image_size) and len(model.sd) == 1238
    _checkpoint(p, drop=lambda k: ".rela_fuse." in k)
    for strict in (False, True):
        model = itf.load_ckpt(p, "cpu", strict=strict)[0]
        assert model.cfg.relation is False and model.cfg.split_weights is strict and model.strict is strict and len(model.sd) == 966
    _checkpoint(p, drop=lambda k: ".rela_fuse." in k, inpaint=True)
    model = itf.load_ckpt(p, "cpu")[0]
    assert model.cfg.relation is False and model.cfg.inpaint_mode is True
    # some but not all: the KeyError of a damaged checkpoint, naming the tensor
    gone = "output_blocks.4.1.transformer_blocks.0.rela_fuse.norm2.bias"
    _checkpoint(p, drop=lambda k: k == gone)
    n = len(_FakeUNet.built)
    with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
        itf.load_ckpt(p, "cpu")
    assert len(_FakeUNet.built) == n                   # refused before a model was built
    sd = recipe.state_dict(TINY, 0)
    assert itf.checkpoint_has_relation(sd, TINY) is True and itf.checkpoint_has_relation(recipe.state_dict(nc.NR_TINY, 0), TINY) is False
    assert itf.checkpoint_has_relation(recipe.state_dict(nc.NR_TINY, 0), nc.NR_TINY) is False


def test_sharded_load_refuses_a_checkpoint_without_rela_fuse(monkeypatch):
    import torch.distributed as dist

    class _M:
        def __init__(self, cfg):
            self.cfg = cfg
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda: 0)
    monkeypatch.setattr(itf, "load_all_models", lambda ckpt, device, strict=None: (_M(nc.NR_TINY), None, None, None, {}))
    with pytest.raises(NotImplementedError, match="without rela_fuse"):
        itf.load_all_models_sharded("x.pth", "cpu")


# ------------------------------------------------------------------------------------------- relations: required, or ignored
class _Untouchable:
    """stands where the engine would: any use is a failure"""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name})")


def _bare_model(cfg):
    m = UNetModel.from_packed(None, cfg, "cpu")
    m.engine = _Untouchable()
    return m


def test_a_relation_model_without_relations_raises_before_the_engine_is_touched():
    inp = {a: T(v) for a, v in recipe.synth_inputs(TINY, 2, 16, n_boxes=4).items()}
    m = _bare_model(TINY)
    g = m.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)
    base = dict(x=inp["x"], timesteps=torch.tensor([1, 1]), context=inp["context"], grounding_input=g, inpainting_extra_input=None,
                grounding_extra_input=None)
    for d in (dict(base), dict(base, relations=None)):
        with pytest.raises(ValueError, match="rela_fuse relation chain.*relations"):
            m(d)
        with pytest.raises(ValueError, match="rela_fuse relation chain.*relations"):
            PLMSSampler(LatentDiffusion(), m).sample(S=2, shape=tuple(inp["x"].shape), input=dict(d), uc=inp["uc"], guidance_scale=7.5)
    with pytest.raises(ValueError, match="rela_fuse relation chain"):
        m.set_conditioning(inp["context"], None, g, 16)
    with pytest.raises(ValueError, match="rela_fuse relation chain"):
        itf.denoise((m, None, None, LatentDiffusion(), {}), inp["context"], inp["uc"], None,
                    dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), inp["x"], steps=2)
    eng = UNetEngine.__new__(UNetEngine)                # no handle, no device: the check comes first
    eng.cfg, eng.handle = TINY, None
    with pytest.raises(ValueError, match="rela_fuse relation chain"):
        eng.set_conditioning(inp["context"], None, inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
    # a model without the chain: no key, None, or a given tensor -- all the same to it
    nr = _bare_model(nc.NR_TINY)
    assert nr.relations_of({}) is None and nr.relations_of(dict(relations=None)) is None and nr.relations_of(dict(relations=inp["relations"])) is None
    assert m.relations_of(dict(relations=inp["relations"])) is inp["relations"]


# ------------------------------------------------------------------------------------------- the negative prompt, the skipped relation phrases
class _SpyEncoder(stubs.StubTextEncoder):
    def __init__(self):
        super().__init__()
        self.calls = []

    def encode(self, texts, return_pooler_output=False):
        self.calls.append((list(texts), return_pooler_output))
        return super().encode(texts, return_pooler_output)


class _Decoder:
    def decode(self, z):
        return torch.zeros(z.shape[0], 3, 4, 4)


@pytest.fixture()
def run_spy(monkeypatch):
    seen = {}

    def fake_denoise(all_models, context, uc, relations, batch, noise, *a, **k):
        seen.update(context=context, uc=uc, relations=relations)
        return noise
    grounding = lambda meta, clip, proc, bs, device=None: dict(boxes=torch.zeros(bs, 30, 4), masks=torch.zeros(bs, 30),
                                                               text_embeddings=torch.zeros(bs, 30, 768))
    monkeypatch.setattr(itf, "denoise", fake_denoise)
    monkeypatch.setattr(itf, "prepare_batch", grounding)
    monkeypatch.setattr(itf, "prepare_batch_multiple", grounding)
    stubs.install_fake_sng_parser()
    return seen


@pytest.mark.parametrize("cfg", [TINY, nc.NR_TINY], ids=["relation", "norel"])
def test_negative_prompt_is_the_unconditional_context(run_spy, cfg):
    class _M:
        pass
    m = _M()
    m.cfg = cfg
    te = _SpyEncoder()
    am = (m, _Decoder(), te, None, {})
    noise = torch.zeros(2, 4, 16, 16)
    meta = dict(prompt="cat sitting on mat", phrases=["cat"], locations=[[0, 0, 1, 1]])
    metab = dict(prompts=["cat sitting on mat", "a quiet street"], phrases=[["cat"], ["street"]], locations=[[[0, 0, 1, 1]]] * 2)
    for run, mt in ((itf.run_one_image, meta), (itf.run_batch_images, metab)):
        for neg, want in ((None, ""), ("lowres, cropped", "lowres, cropped")):
            te.calls.clear()
            args = dict(batch_size=2, guidance_scale=7.5, no_plms=False)
            if neg is not None:
                args["negative_prompt"] = neg
            run(am, args, dict(mt), noise)
            singles = [c[0] for c in te.calls if len(c[0]) == 1 and not c[1]]
            assert singles == [[want]], te.calls
            assert torch.equal(run_spy["uc"], stubs.StubTextEncoder().encode([want]).repeat(2, 1, 1))
            pooled = [c for c in te.calls if c[1]]                      # the relation phrases
            if cfg.relation:
                assert pooled and run_spy["relations"] is not None and tuple(run_spy["relations"].shape) == (2, 10, 768)
            else:
                assert not pooled and run_spy["relations"] is None
    # per call, not sticky through the config dict that _run updates: the next call without one encodes "" again
    te.calls.clear()
    itf.run_one_image(am, dict(batch_size=2, guidance_scale=7.5, no_plms=False), dict(meta), noise)
    assert [""] in [c[0] for c in te.calls]
    with pytest.raises(TypeError, match="negative_prompt"):
        itf.run_one_image(am, dict(batch_size=2, guidance_scale=7.5, no_plms=False, negative_prompt=["a"]), dict(meta), noise)


def test_gligen_inference_run_passes_the_negative_prompt_on(monkeypatch):
    seen = []
    monkeypatch.setattr(itf, "run_one_image", lambda am, args, m, noise, clip, proc, device=None: seen.append(dict(args)) or [])
    monkeypatch.setitem(gi._MODELS, "ck", (type("M", (), {"first_conv_type": "SD"})(), None, None, None, {}))
    meta = dict(ckpt="ck", prompt="p", phrases=["a"], locations=[[0, 0, 1, 1]])
    noise = torch.zeros(1, 4, 16, 16)
    gi.run(meta, dict(batch_size=1, device="cpu", negative_prompt="lowres"), noise, clip_model=object(), clip_processor=object())
    gi.run(meta, dict(batch_size=1, device="cpu"), noise, clip_model=object(), clip_processor=object())
    gi.run(meta, dict(batch_size=1, device="cpu", negative_prompt=None), noise, clip_model=object(), clip_processor=object())
    assert seen[0]["negative_prompt"] == "lowres" and "negative_prompt" not in seen[1] and "negative_prompt" not in seen[2]
