"""The UNet without the rela_fuse chain (``UNetConfig.relation = False``, gl_unet_config.no_relation: the upstream GLIGEN transformer block that
every public GLIGEN checkpoint was trained on) on the GPU: the tiny UNet against the reference's pre-modification model
(tests/golden/norel_*.npz) in default and strict mode, the PLMS run without a "relations" key, CFG batching, a relation handle next to a
no-relation one, full-width levels against tests/norel_ref.py, the conditioning entries with a NULL relations pointer, and the interface
boundary on synthetic checkpoints without rela_fuse tensors."""
import dataclasses
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import golden_cases as gc
import norel_cases as nc
import norel_ref
import stubs
from layoutllm_t2i_amd import recipe, weights
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, UNetConfig, VAEConfig
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, TextImageGroundingNetInput, UNetModel
from layoutllm_t2i_amd.sampler import PLMSSampler
from test_gpu_model import rel_l2, report

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


_models = {}


def get_model(family="text", split_weights=False, fresh=False):
    key = (family, split_weights)
    if fresh or key not in _models:
        base = {"text": nc.NR_TINY, "text_image": nc.NR_TI_TINY, "inpaint": nc.NR_IP_TINY}[family]
        m = UNetModel(dataclasses.replace(base, split_weights=split_weights), recipe.state_dict(base, 0), device=DEV,
                      sd_first_conv=None if base.inpaint_mode else recipe.sd_first_conv(base, 0))
        m.grounding_tokenizer_input = TextImageGroundingNetInput() if family == "text_image" else GroundingNetInput()
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def _batch(cfg, inp):
    if cfg.grounding == "text_image":
        return {k: inp[k] for k in nc.TI_KEYS}
    return dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])


def _golden_call(model, case, inp, **more):
    """the upstream ``input`` dict: no "relations" key (``more`` adds one)"""
    model.fuser_scale = case["scale"]
    model.first_conv_type = "SD" if case["sdconv"] else "GLIGEN"
    g = model.grounding_tokenizer_input.prepare(_batch(model.cfg, inp))
    d = dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"],
             inpainting_extra_input=inp.get("extra"), grounding_extra_input=None, **more)
    if case["grounding"] == "real":
        d["grounding_input"] = g
    else:
        d["context"] = inp["uc"]
    try:
        return model(d)
    finally:
        model.first_conv_type = "GLIGEN"


# ------------------------------------------------------------------------------------------- whole model: tiny UNet vs the reference
@pytest.mark.parametrize("case", nc.UNET_CASES, ids=[c["name"] for c in nc.UNET_CASES])
def test_tiny_unet_matches_reference_golden(case):
    """default mode, the bound tests/test_gpu_model.py / test_gpu_ti.py / test_gpu_inpaint9.py apply to the sibling cases; graph replay ==
    eager bitwise; a given relations tensor is ignored bit for bit"""
    model = get_model(case["family"])
    inp = {a: T(v) for a, v in nc.case_inputs(case).items()}
    ref = T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"])
    out = _golden_call(model, case, inp)
    r = report(case["name"], out, ref)
    assert r < 2.1e-3, r
    model.engine.use_graphs = False
    try:
        eager = _golden_call(model, case, inp)
    finally:
        model.engine.use_graphs = True
    assert torch.equal(eager, out), "graph replay == eager"
    assert torch.equal(_golden_call(model, case, inp, relations=inp["relations"]), out), "a given relations tensor is ignored"
    assert model.engine.cond["R"] == 0


@pytest.mark.parametrize("case", nc.UNET_CASES, ids=[c["name"] for c in nc.UNET_CASES])
def test_tiny_unet_strict_matches_reference_golden(case):
    """strict mode on a split_weights handle, the bounds of the sibling cases in strict mode"""
    model = get_model(case["family"], True)
    inp = {a: T(v) for a, v in nc.case_inputs(case).items()}
    ref = T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"])
    model.set_strict(True)
    try:
        out = _golden_call(model, case, inp)
        model.engine.use_graphs = False
        eager = _golden_call(model, case, inp)
    finally:
        model.engine.use_graphs = True
        model.set_strict(False)
    r = report(case["name"] + " strict", out, ref)
    outside = float(((out.float().cpu() - ref).abs() > 1e-4 + 1e-3 * ref.abs()).float().mean())
    print(f"[{case['name']} strict] outside rtol 1e-3 / atol 1e-4: {outside * 100:.2f} %")
    assert r < 5e-5 and outside < 0.01, (r, outside)
    assert torch.equal(eager, out), "graph replay == eager in strict mode"


def test_lazy_strict_hoists_on_a_no_relation_handle():
    """a split handle conditioned in DEFAULT mode computes the strict hoists with the first strict forward: the bits of conditioning in strict mode"""
    model = get_model("text", True)
    case = nc.by_name("norel_unet_tiny_cond")
    inp = {a: T(v) for a, v in nc.case_inputs(case).items()}
    eng, x = model.engine, inp["x"].to(DEV)
    model.set_strict(False)
    eng.set_conditioning(inp["context"], None, inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
    eng.forward(x, 481.0, 1.0, False, 1)
    try:
        eng.set_option(50, 1)
        lazy = eng.forward(x, 481.0, 1.0, False, 1).clone()
        eng.set_conditioning(inp["context"], None, inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
        assert torch.equal(eng.forward(x, 481.0, 1.0, False, 1), lazy)
    finally:
        model.set_strict(False)


def test_plms_tiny_matches_reference_golden():
    """the 10-step golden (CFG 7.5, B = 2, alpha_type [0.3, 0, 0.7]) through PLMSSampler with the upstream input dict, no "relations" key: the
    bound of tests/test_gpu_model.py::test_plms_tiny_matches_reference_golden"""
    case = nc.by_name("norel_plms_tiny")
    inp = {a: T(v) for a, v in nc.case_inputs(case).items()}
    model = get_model()
    model.first_conv_type = "GLIGEN"
    sampler = PLMSSampler(LatentDiffusion(device=DEV), model, alpha_generator_func=partial(itf.alpha_generator, type=case["alpha_type"]),
                          set_alpha_scale=itf.set_alpha_scale)
    g = model.grounding_tokenizer_input.prepare(_batch(model.cfg, inp), None)
    d = dict(x=inp["x"].to(DEV), timesteps=None, context=inp["context"], grounding_input=g, inpainting_extra_input=None, grounding_extra_input=None)
    assert "relations" not in d
    out = sampler.sample(S=case["S"], shape=tuple(inp["x"].shape), input=d, uc=inp["uc"], guidance_scale=case["guidance"])
    assert model.first_conv_type == "SD", "restore_first_conv_from_SD must stick (openaimodel.py:393-411)"
    model.first_conv_type = "GLIGEN"
    r = report("norel_plms_tiny", out, T(np.load(os.path.join(GOLD, "norel_plms_tiny.npz"))["out"]))
    assert r < 3.1e-3, r


# ------------------------------------------------------------------------------------------- batching
def test_cfg_batched_2b_equals_two_calls():
    """[cond ; uncond] as one 2B batch == two B-sized calls, as tests/test_gpu_model.py::test_cfg_batched_2b_equals_two_calls asserts, with the
    shared cond / uncond prefix (option 44) on and off, fuser on and off (at scale 0 attn2 is the first op that reads the conditioning)"""
    eng = get_model().engine
    inp = {a: T(v) for a, v in nc.case_inputs(nc.by_name("norel_unet_tiny_cond")).items()}
    x, z, cat = inp["x"].to(DEV), torch.zeros_like, (lambda a, b: torch.cat([a, b], 0))
    for scale in (1.0, 0.0):
        eng.set_conditioning(inp["context"], None, inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
        ec = eng.forward(x, 981.0, scale, False, 1).clone()
        eng.set_conditioning(inp["uc"], None, z(inp["boxes"]), z(inp["masks"]), z(inp["positive_embeddings"]), 16)
        eu = eng.forward(x, 981.0, scale, False, 1).clone()
        assert rel_l2(ec, eu) > 1e-2                        # the two halves are different problems
        eng.set_conditioning(cat(inp["context"], inp["uc"]), None, cat(inp["boxes"], z(inp["boxes"])), cat(inp["masks"], z(inp["masks"])),
                             cat(inp["positive_embeddings"], z(inp["positive_embeddings"])), 16)
        try:
            for share in (1, 0):
                eng.set_option(44, share)
                e2 = eng.forward(x, 981.0, scale, False, 2).clone()
                rc, ru = rel_l2(e2[:2], ec), rel_l2(e2[2:], eu)
                print(f"[norel 2B scale={scale} share={share}] rel_l2 cond {rc:.2e} uncond {ru:.2e}")
                assert rc < 1e-6 and ru < 1e-6, (scale, share, rc, ru)
        finally:
            eng.clear_options()


def test_fewer_launches_and_no_relation_buffers():
    """a strict subset of the relation handle's launches plus one unfused LayerNorm per transformer block (16 of them in the tiny UNet)"""
    nr = get_model(fresh=True).engine                   # fresh: the pools of the two handles have seen the same shapes
    rl = UNetModel(TINY, recipe.state_dict(TINY, 0), device=DEV).engine
    inp = {a: T(v) for a, v in nc.case_inputs(nc.by_name("norel_unet_tiny_cond")).items()}
    x = inp["x"].to(DEV)
    for eng, rel in ((nr, None), (rl, inp["relations"])):
        eng.set_conditioning(inp["context"], rel, inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
    n_st = len(nr.plan.st_layers())
    for scale in (1.0, 0.0):
        counts = []
        for eng in (nr, rl):
            eng.use_graphs = False
            try:
                eng.forward(x, 501.0, scale, False, 1)
            finally:
                eng.use_graphs = True
            counts.append(eng.num_launches())
        print(f"[norel launches fuser={'on' if scale else 'off'}] no-relation {counts[0]} relation {counts[1]} ({n_st} transformer blocks)")
        # per block the relation chain is 9 launches (LayerNorm statistics, box pooling, q, attention, to_out, norm2, ff1, ff2, merge with the
        # fused LayerNorm(norm2)); without it LayerNorm(norm2) is a launch of its own
        assert counts[0] == counts[1] - 9 * n_st + n_st, counts
    assert nr.pool_bytes() < rl.pool_bytes()


# ------------------------------------------------------------------------------------------- next to a relation handle
def test_relation_and_no_relation_handles_alternate():
    """the relation handle's output on unet_tiny_cond stays bit-identical to what it was before the no-relation handle existed, and within its
    own bound of the relation golden; the no-relation handle's output does not move either"""
    case = next(c for c in gc.CASES if c["name"] == "unet_tiny_cond")
    inp = {a: T(v) for a, v in gc.case_inputs(case).items()}
    rel = UNetModel(TINY, recipe.state_dict(TINY, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(TINY, 0))
    x = inp["x"].to(DEV)

    def run_rel():
        rel.engine.set_conditioning(inp["context"], inp["relations"], inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
        return rel.engine.forward(x, 981.0, 1.0, False, 1).clone()
    before = run_rel()
    assert report("unet_tiny_cond (relation handle)", before, T(np.load(os.path.join(GOLD, "unet_tiny_cond.npz"))["out"])) < 2.1e-3
    nr = get_model(fresh=True)

    def run_nr():
        nr.engine.set_conditioning(inp["context"], None, inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
        return nr.engine.forward(x, 981.0, 1.0, False, 1).clone()
    first = run_nr()
    assert report("norel_unet_tiny_cond (fresh handle)", first, T(np.load(os.path.join(GOLD, "norel_unet_tiny_cond.npz"))["out"])) < 2.1e-3
    assert rel_l2(first, before) > 0.1
    for _ in range(2):
        assert torch.equal(run_rel(), before)
        assert torch.equal(run_nr(), first)
    rel.engine.use_graphs = False
    assert torch.equal(run_rel(), before)


# ------------------------------------------------------------------------------------------- the C entries
def test_null_relations_pointer_per_handle_kind():
    """gl_set_conditioning / _hw / _ti: a NULL relations pointer (and any R) is accepted on a no-relation handle and GL_ERR_BAD_ARG on a relation
    handle, before anything is launched"""
    d = lambda t: t.to(DEV).contiguous()
    inp = {a: d(T(v)) for a, v in nc.case_inputs(nc.by_name("norel_unet_tiny_cond")).items()}
    ti = {a: d(T(v)) for a, v in nc.case_inputs(nc.by_name("norel_ti_unet_tiny_s1")).items()}
    nr, nrti = get_model().engine, get_model("text_image").engine
    rl = UNetModel(TINY, recipe.state_dict(TINY, 0), device=DEV).engine
    rlti = UNetModel(dataclasses.replace(TINY, grounding="text_image"), recipe.state_dict(dataclasses.replace(TINY, grounding="text_image"), 0),
                     device=DEV).engine
    p = lambda t: t.data_ptr()
    text = lambda e, rel, R: (e.handle, p(inp["context"]), rel, p(inp["boxes"]), p(inp["masks"]), p(inp["positive_embeddings"]), 2, 77, R)
    tiargs = lambda e, rel, R: (e.handle, p(ti["context"]), rel, p(ti["boxes"]), p(ti["masks"]), p(ti["text_masks"]), p(ti["image_masks"]),
                                p(ti["text_embeddings"]), p(ti["image_embeddings"]), 2, 77, R, 16, 16, None)
    l = nr._lib
    with torch.cuda.device(DEV):
        for R in (0, 10, -3):
            assert l.gl_set_conditioning(*text(nr, None, R), 16, None) == 0
            assert l.gl_set_conditioning_hw(*text(nr, None, R), 8, 16, None) == 0
            assert l.gl_set_conditioning_ti(*tiargs(nrti, None, R)) == 0
        assert l.gl_set_conditioning(*text(nr, p(inp["relations"]), 10), 16, None) == 0            # a given pointer is ignored
        for R in (0, 10):
            assert l.gl_set_conditioning(*text(rl, None, R), 16, None) == -1
            assert l.gl_set_conditioning_hw(*text(rl, None, R), 8, 16, None) == -1
            assert l.gl_set_conditioning_ti(*tiargs(rlti, None, R)) == -1
        assert l.gl_set_conditioning(*text(rl, p(inp["relations"]), 0), 16, None) == -1           # R <= 0 with a pointer
        assert l.gl_set_conditioning(*text(rl, p(inp["relations"]), 10), 16, None) == 0
        torch.cuda.synchronize()
    # the python face puts the handles back into a known state (its own bookkeeping of the conditioning)
    nr.set_conditioning(inp["context"], None, inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
    ref = T(np.load(os.path.join(GOLD, "norel_unet_tiny_cond.npz"))["out"])
    assert rel_l2(nr.forward(inp["x"], 981.0, 1.0, False, 1), ref) < 2.1e-3


# ------------------------------------------------------------------------------------------- full-width levels
# One-level plans, each with the width and head dim of one level of the full configuration (model_channels 320, 8 heads): what
# tests/test_gpu_model.py's LEVELS and tests/test_gpu_ti.py::test_default_mode_full_width_level_vs_ti_ref call a full-width level
LEVELS = [("L0_c320_d40", (1,), 40), ("L1_c640_d80", (2,), 80), ("L2_c1280_d160", (4,), 160)]


@pytest.mark.parametrize("name,mult,d", LEVELS, ids=[l[0] for l in LEVELS])
def test_default_mode_full_width_levels_vs_norel_ref(name, mult, d):
    """model_channels 320, 8 heads, one ResBlock, ONE level of width 320 / 640 / 1280 (d = 40 / 80 / 160) with its transformer, middle block
    and skip-concat ResBlocks, 16 x 16, B = 2 as a [cond ; uncond] batch over the two latents, default mode, against tests/norel_ref.py on the
    same fp16-representable weights: the bound and the method of tests/test_gpu_ti.py::test_default_mode_full_width_level_vs_ti_ref (whose
    plan is the first of these).  The weights are drawn on the device (weights.random_state_dict: the recipe's scaling rules), which keeps
    each case at a few seconds.

    The bound belongs to one-level plans: it is 1.5 x what they measure (4.3e-4 ... 5.0e-4 on this path and on the relation path alike).  A
    three-level plan of the same widths (10 transformer blocks instead of 4) measures 7.4e-4 ... 7.8e-4 on BOTH paths, the relation handle's
    untouched launch sequence included (profiles/norel_parity.txt): depth, not the path, and not what this bound was made for."""
    cfg = UNetConfig(image_size=16, model_channels=320, channel_mult=mult, attention_resolutions=(1,), num_res_blocks=1, relation=False)
    sd = {k: (v.half().float() if v.dim() >= 2 else v) for k, v in weights.random_state_dict(cfg, DEV, seed=3).items()}
    model = UNetModel(cfg, sd, device=DEV)
    assert {l.d_head for l in model.engine.plan.st_layers()} == {d}
    inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, 2, 16, n_boxes=8, n_rel=3, seed=4321).items()}
    h16 = lambda t: t.half().float()
    g = {k: inp[k] for k in nc.TEXT_KEYS}
    gn = norel_ref.null_grounding(g)
    cat = lambda a, b: torch.cat([a, b], 0)
    model.engine.set_conditioning(cat(inp["context"], inp["uc"]), None, cat(g["boxes"], gn["boxes"]), cat(g["masks"], gn["masks"]),
                                  cat(g["positive_embeddings"], gn["positive_embeddings"]), 16)
    out = model.engine.forward(h16(inp["x"]).to(DEV), 481.0, 1.0, False, 2).clone()
    t = torch.full((2,), 481, dtype=torch.long)
    osd = {k: v.cpu() for k, v in sd.items()}
    with torch.no_grad():
        torch.set_num_threads(min(16, max(1, os.cpu_count() or 1)))
        rc = norel_ref.unet_forward(osd, cfg, h16(inp["x"]), t, h16(inp["context"]), g)
        ru = norel_ref.unet_forward(osd, cfg, h16(inp["x"]), t, h16(inp["uc"]), gn)
    r = report(f"norel {name}_16x16", out, cat(rc, ru))
    assert r < 7.5e-4, r
    del model
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- the boundary
VAE8 = VAEConfig(ch=64, ch_mult=(1, 1, 2, 2), num_res_blocks=1)       # three downsamples: 16 x 16 latents <-> 128 x 128 images
LOC = [[0.10, 0.10, 0.50, 0.55], [0.55, 0.20, 0.90, 0.70]]
ARGS = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)


def _write_checkpoint(path, inpaint=False):
    """stubs.write_synthetic_checkpoint's container as GLIGEN's own checkpoints have it: no ``*.rela_fuse.*`` tensor in ``model``; with
    ``inpaint`` also ``inpaint_mode: True``, a [mc, 9, 3, 3] first conv and no SD conv file; the VAE encoder (for the input image)"""
    ck = stubs.write_synthetic_checkpoint(path, TINY, VAE8, max_relations=10, with_sd_conv=not inpaint)
    cfg = nc.NR_IP_TINY if inpaint else nc.NR_TINY
    if inpaint:
        ck["config_dict"]["_content"]["model"]["params"]["inpaint_mode"] = True
    ck["model"] = {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in recipe.state_dict(cfg, 0).items()}
    assert len(ck["model"]) == 966
    ck["autoencoder"].update({k: T(np.asarray(v)) for k, v in recipe.vae_encoder_state_dict(VAE8, 0).items()})
    torch.save(ck, path)


class _NoRelationPhrases:
    """stands for sng_parser: a checkpoint without rela_fuse must not parse the prompt"""

    def parse(self, prompt):
        raise AssertionError("the scene-graph parser was called for a model without the relation chain")


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt_norel")
    pt, pi = str(d / "text" / "tiny_gligen_text.pth"), str(d / "inpaint" / "tiny_gligen_inpainting_text.pth")
    for p in (pt, pi):
        os.makedirs(os.path.dirname(p))
    _write_checkpoint(pt)
    _write_checkpoint(pi, inpaint=True)
    saved = sys.modules.get("sng_parser")
    sys.modules["sng_parser"] = _NoRelationPhrases()
    try:
        yield pt, pi, itf.load_all_models(pt, DEV), itf.load_all_models(pi, DEV), stubs.toy_clip().to(DEV), stubs.ToyProcessor(), d
    finally:
        if saved is not None:
            sys.modules["sng_parser"] = saved
        else:
            del sys.modules["sng_parser"]


def _input_image():
    from PIL import Image
    return Image.fromarray((np.clip(recipe.uniform("gpunorel.img", (40, 56, 3), 4), 0, 1) * 255).astype(np.uint8))


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_text_checkpoint_through_run_batch_images(loaded):
    pt, pi, am, ami, clip, proc, d = loaded
    model = am[0]
    assert model.cfg.relation is False and not model.cfg.inpaint_mode and model.first_conv_restorable
    assert not any("rela_fuse" in k for k in model.engine.W) and isinstance(model.grounding_tokenizer_input, GroundingNetInput)
    meta = dict(prompts=["cat sitting on mat", "a quiet street"], phrases=[["cat", "mat"], ["street"]], locations=[LOC, [[0.0, 0.5, 1.0, 1.0]]],
                alpha_type=[0.5, 0.0, 0.5])
    noise = T(recipe.normal("gpunorel.noise", (2, 4, 16, 16), 9))

    def run(**more):
        model.first_conv_type = "GLIGEN"
        return itf.run_batch_images(am, dict(ARGS, **more), dict(meta), noise.clone().to(DEV), clip, proc, device=DEV)
    a = run()
    assert len(a) == 2 and all(im.size == (128, 128) and im.mode == "RGB" for im in a)
    assert model.first_conv_type == "SD"                # alpha_type [0.5, 0, 0.5] ran scale-0 steps
    assert _same(a, run()), "the same noise gives the same images"
    assert not _same(a, run(negative_prompt="lowres, cropped, worst quality")), "a negative prompt changes the images"
    assert _same(a, run()), "... for that call only"
    rect = itf.run_batch_images(am, dict(ARGS), dict(meta), torch.randn(2, 4, 8, 16).to(DEV), clip, proc, device=DEV)
    assert len(rect) == 2 and rect[0].size == (128, 64)


def test_inpaint_checkpoint_through_run_one_image(loaded):
    pt, pi, am, ami, clip, proc, d = loaded
    model = ami[0]
    assert model.cfg.relation is False and model.cfg.inpaint_mode and model.cfg.first_conv_in == 9 and not model.first_conv_restorable
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5], input_image=_input_image())
    noise = T(recipe.normal("gpunorel.noise", (2, 4, 16, 16), 9))

    def run(**more):
        torch.manual_seed(11)                           # the q_sample noise of the masked steps and the VAE posterior draw
        return itf.run_one_image(ami, dict(ARGS, **more), dict(meta), noise.clone().to(DEV), clip, proc, device=DEV)
    a = run()
    assert len(a) == 2 and all(im.size == (128, 128) and im.mode == "RGB" for im in a)
    assert _same(a, run()), "the same seed gives the same images"
    assert not _same(a, run(negative_prompt="lowres, cropped, worst quality")), "a negative prompt changes the images"
    with pytest.raises(ValueError, match="input_image"):
        itf.run_one_image(ami, dict(ARGS), {k: v for k, v in meta.items() if k != "input_image"}, noise.clone().to(DEV), clip, proc, device=DEV)


def test_gligen_inference_run(loaded, tmp_path):
    pt, pi, am, ami, clip, proc, d = loaded
    from layoutllm_t2i_amd import gligen_inference as gi
    gi._MODELS[pt] = am
    try:
        meta = dict(ckpt=pt, prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, save_folder_name="norel")
        cfg = dict(batch_size=1, guidance_scale=7.5, no_plms=False, folder=str(tmp_path), device=DEV, steps=4)
        noise = T(recipe.normal("gpunorel.noise1", (1, 4, 16, 16), 9))
        a = gi.run(meta, dict(cfg), starting_noise=noise.clone().to(DEV), clip_model=clip, clip_processor=proc)
        assert len(a) == 1 and a[0].size == (128, 128) and os.path.exists(tmp_path / "norel" / "0.png")
        assert _same(a, gi.run(meta, dict(cfg), starting_noise=noise.clone().to(DEV), clip_model=clip, clip_processor=proc))
        b = gi.run(meta, dict(cfg, negative_prompt="lowres, cropped, worst quality"), starting_noise=noise.clone().to(DEV), clip_model=clip,
                   clip_processor=proc)
        assert b[0].size == (128, 128) and not _same(a, b)
        torch.manual_seed(3)
        c = gi.run(meta, dict(cfg, height=64, width=128), clip_model=clip, clip_processor=proc)      # sizes its own noise
        assert c[0].size == (128, 64)
    finally:
        gi._MODELS.pop(pt, None)


def test_strict_load_of_a_checkpoint_without_rela_fuse(loaded):
    pt, pi, am, ami, clip, proc, d = loaded
    ams = itf.load_all_models(pt, DEV, strict=True)
    assert ams[0].strict and ams[0].cfg.split_weights and ams[0].cfg.relation is False
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5])
    noise = T(recipe.normal("gpunorel.noise", (2, 4, 16, 16), 9))
    lat = {}
    for tag, models in (("strict", ams), ("default", am)):
        dec = models[1].decode
        models[1].decode = lambda z, dec=dec, tag=tag: dec(lat.setdefault(tag, z.clone()))
        models[0].first_conv_type = "GLIGEN"
        try:
            out = itf.run_one_image(models, dict(ARGS), dict(meta), noise.clone().to(DEV), clip, proc, device=DEV)
        finally:
            models[1].decode = dec
        assert len(out) == 2 and out[0].size == (128, 128)
    r = rel_l2(lat["default"], lat["strict"])
    print(f"[norel boundary] default vs strict latent rel_l2 = {r:.3e}")
    # as tests/test_gpu_inpaint9.py reasons for its twin: the default latent within 2.7e-3 of the fp32 pipeline, the strict one within 1e-4
    assert 0 < r < 2.7e-3 + 1e-4, r
