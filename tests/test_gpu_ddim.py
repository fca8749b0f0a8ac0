"""The DDIM sampler on the GPU: gl_ddim_update against the torch fp32 expression (bitwise), gl_ddim_step against its two parts (bitwise),
``DDIMSampler`` against the latents of the reference's own DDIMSampler with its noise draws replayed (tests/golden/ddim_*.npz) in default
and strict mode, against tests/ddim_ref.py where the reference cannot run (guidance on the relation UNet, a rectangular masked latent),
determinism, and the public switch on a synthetic checkpoint.

The golden bound is relative, not a number: in the same run the existing ``PLMSSampler`` is measured on its golden of the same model and
mode (``norel_plms_tiny`` / ``plms_tiny``), and DDIM must stay below twice that error -- DDIM has no Adams-Bashforth history that amplifies
an eps error, so it should be no worse than PLMS; the factor 2 absorbs the case-to-case spread.  Both values are printed
(``[ddim_parity] ...``; profiles/ddim_parity.txt holds a recorded run)."""
import dataclasses
import functools
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import ddim_cases as dc
import ddim_ref
import golden_cases as gc
import norel_cases as nc
import stubs
import test_oracle_golden as tog
from layoutllm_t2i_amd import _lib, host, ops, recipe
from layoutllm_t2i_amd import gligen_inference as gi
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel
from layoutllm_t2i_amd.sampler import DDIMSampler, PLMSSampler

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------- the kernel, bit for bit
COEFS = host.ddim_step_coefs(host.make_ddim_schedule(10, host.alphas_cumprod(), "uniform", 1.0), 6)      # five float32 scalars, sigma > 0
# [1] and [1, 3, 7, 13] (273 elements: two blocks and a tail) take the scalar path; [1, 4, 3, 5] (60) and [2, 4, 16, 16] the float4 path
SHAPES = [(1,), (1, 4, 3, 5), (2, 4, 16, 16), (1, 3, 7, 13)]


def _torch_ddim(eps, x, noise, reps, guidance, coefs):
    """ddim.py:115-135 as the reference writes it, on the device, every scalar a float32 tensor (``torch.full``)"""
    full = lambda v: torch.full((1,) * x.dim(), v, device=x.device)
    sqrt_at, s1m, sqrt_aprev, dir_coef, sigma = (full(v) for v in coefs)
    if reps == 2:
        e_c, e_u = eps[:eps.shape[0] // 2], eps[eps.shape[0] // 2:]
        e = e_u + guidance * (e_c - e_u)
    else:
        e = eps
    e = e.reshape(x.shape)
    pred_x0 = (x - s1m * e) / sqrt_at
    dir_xt = dir_coef * e
    x_prev = sqrt_aprev * pred_x0 + dir_xt
    if noise is not None:
        x_prev = x_prev + sigma * noise
    return x_prev, pred_x0


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("reps", [1, 2])
def test_ddim_update_is_bitwise_the_torch_expression(shape, reps):
    tag = "ddim.k." + "x".join(map(str, shape))
    x = T(recipe.normal(tag + ".x", shape, 3)).to(DEV)
    eps = T(recipe.normal(tag + ".eps", (reps * shape[0],) + tuple(shape[1:]), 3)).to(DEV)
    noise = T(recipe.normal(tag + ".noise", shape, 3)).to(DEV)
    kw = dict(zip(("sqrt_at", "s1m", "sqrt_aprev", "dir_coef", "sigma"), COEFS))
    for with_noise in (False, True):
        n = noise if with_noise else None
        coefs = COEFS if with_noise else COEFS[:4] + (0.0,)
        k = dict(kw, sigma=coefs[4], noise=n, guidance=7.5)
        ref, ref_p = _torch_ddim(eps, x, n, reps, 7.5, coefs)
        if not with_noise:
            # NULL noise skips the term: the bits of the reference's x_prev + 0 * randn
            assert torch.equal(ref, _torch_ddim(eps, x, noise, reps, 7.5, coefs)[0])
        for in_place in (False, True):
            for with_pred in (False, True):
                xin = x.clone()
                out = xin if in_place else torch.full_like(x, float("nan"))
                pred = torch.full_like(x, float("nan")) if with_pred else None
                got = ops.ddim_update(eps, xin, out, pred_x0=pred, **k)
                assert got is out and torch.equal(out, ref), (with_noise, in_place, with_pred, float((out - ref).abs().max()))
                assert pred is None or torch.equal(pred, ref_p)
                assert in_place or torch.equal(xin, x)


def test_ddim_update_on_unaligned_pointers_and_bad_arguments():
    """a 4-byte-aligned view takes the scalar path whatever n is; what the entry refuses"""
    base = {k: T(recipe.normal(f"ddim.k.un.{k}", (2 * 512 + 1,), 3)).to(DEV) for k in ("x", "eps", "noise", "out", "pred")}
    x, noise, out, pred = (base[k][1:257] for k in ("x", "noise", "out", "pred"))
    eps = base["eps"][1:513]
    kw = dict(zip(("sqrt_at", "s1m", "sqrt_aprev", "dir_coef", "sigma"), COEFS))
    ops.ddim_update(eps, x, out, noise=noise, guidance=3.0, pred_x0=pred, **kw)
    ref, ref_p = _torch_ddim(eps.reshape(2, 256), x.reshape(1, 256), noise.reshape(1, 256), 2, 3.0, COEFS)
    assert torch.equal(out, ref.reshape(-1)) and torch.equal(pred, ref_p.reshape(-1))
    assert torch.equal(base["out"][257:], T(recipe.normal("ddim.k.un.out", (1025,), 3))[257:].to(DEV)), "nothing written behind the view"
    with pytest.raises(ValueError):
        ops.ddim_update(base["eps"][:300], x, out, **kw)                  # neither n nor 2n
    with pytest.raises(ValueError):
        ops.ddim_update(eps, x, base["out"][:100], **kw)
    with pytest.raises(_lib.HipLibraryError):
        ops.ddim_update(eps.cpu(), x, out, **kw)
    lib = _lib.lib()
    assert lib.gl_ddim_update(eps.data_ptr(), x.data_ptr(), None, 3, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 256, out.data_ptr(), None, None) != 0
    assert lib.gl_ddim_update(None, x.data_ptr(), None, 1, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 256, out.data_ptr(), None, None) != 0
    assert lib.gl_ddim_update(eps.data_ptr(), x.data_ptr(), None, 1, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0, out.data_ptr(), None, None) != 0


# ------------------------------------------------------------------------------------------- models
_models = {}


def get_model(unet, strict=False):
    key = (unet, strict)
    if key not in _models:
        base = nc.NR_TINY if unet == "norel" else TINY
        m = UNetModel(dataclasses.replace(base, split_weights=strict), recipe.state_dict(base, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(base, 0))
        m.grounding_tokenizer_input = GroundingNetInput()
        if strict:
            m.set_strict(True)
        _models[key] = m
    return _models[key]


def _input(model, inp):
    g = model.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)
    return dict(x=inp["x"].to(DEV), timesteps=None, context=inp["context"], relations=inp["relations"], grounding_input=g,
                inpainting_extra_input=None, grounding_extra_input=None)


def _callbacks(alpha_type):
    return dict(alpha_generator_func=partial(itf.alpha_generator, type=alpha_type), set_alpha_scale=itf.set_alpha_scale)


def run_ddim(model, case, inp, randn_like=None):
    """``DDIMSampler.sample`` on the case (eta and the discretisation through the constructor); ``randn_like``: the stand-in for the run"""
    model.first_conv_type = "GLIGEN"
    s = DDIMSampler(LatentDiffusion(device=DEV), model, eta=case["eta"], discretize=case["discretize"], **_callbacks(case["alpha_type"]))
    with dc.patched_randn_like(randn_like if randn_like is not None else torch.randn_like):
        out = s.sample(S=case["S"], shape=tuple(inp["x"].shape), input=_input(model, inp), uc=inp["uc"], guidance_scale=case["guidance"],
                       mask=inp.get("mask"), x0=inp.get("x0"))
    model.first_conv_type = "GLIGEN"
    return out


@functools.lru_cache(maxsize=None)
def plms_error(unet, strict):
    """rel-L2 of the existing PLMSSampler on its golden of the same model and mode (measured once per module run)"""
    case = dc.plms_case(dict(unet=unet))
    inp = {a: T(v) for a, v in (nc if unet == "norel" else gc).case_inputs(case).items()}
    model = get_model(unet, strict)
    model.first_conv_type = "GLIGEN"
    s = PLMSSampler(LatentDiffusion(device=DEV), model, **_callbacks(case["alpha_type"]))
    out = s.sample(S=case["S"], shape=tuple(inp["x"].shape), input=_input(model, inp), uc=inp["uc"], guidance_scale=case["guidance"])
    model.first_conv_type = "GLIGEN"
    return rel_l2(out, T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]))


def _parity(name, mode, r_ddim, r_plms):
    print(f"[ddim_parity] {name:28s} {mode:8s} r_ddim = {r_ddim:.3e}   r_plms = {r_plms:.3e}   ratio = {r_ddim / r_plms:.2f}   (bound: ratio < 2)")


# ------------------------------------------------------------------------------------------- fused step == its two parts
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_ddim_step_equals_forward_plus_update(graphs):
    assert _lib.lib().gl_sizeof_ddim_step_args() == __import__("ctypes").sizeof(_lib.DdimStepArgs)
    model = get_model("rel")
    eng = model.engine
    inp = {k: T(v) for k, v in recipe.synth_inputs(TINY, 2, 16, n_boxes=4, n_rel=3, seed=21).items()}
    z, cat = torch.zeros_like, lambda p, q: torch.cat([p, q], 0)
    eng.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
                         cat(inp["masks"], z(inp["masks"])), cat(inp["positive_embeddings"], z(inp["positive_embeddings"])), 16)
    x = inp["x"].to(DEV).contiguous()
    noise = T(recipe.normal("ddim.step.noise", tuple(x.shape), 3)).to(DEV)
    kw = dict(zip(("sqrt_at", "s1m", "sqrt_aprev", "dir_coef", "sigma"), COEFS))
    eng.use_graphs = graphs
    try:
        for n in (noise, None):
            k = dict(kw, sigma=COEFS[4] if n is not None else 0.0)
            x_out, pred = torch.empty_like(x), torch.empty_like(x)
            eng.ddim_step(x, x_out, t=601.0, reps=2, guidance=7.5, fuser_scale=1.0, sd_conv=False, noise=n, pred_x0=pred, **k)
            eps = eng.forward(x, 601.0, 1.0, False, 2).clone()
            pred2 = torch.empty_like(x)
            x2 = ops.ddim_update(eps, x, torch.empty_like(x), noise=n, guidance=7.5, pred_x0=pred2, **k)
            assert torch.isfinite(x2).all() and torch.equal(x_out, x2) and torch.equal(pred, pred2)
            # the in-place form the sampler uses, without pred_x0
            xa = x.clone()
            eng.ddim_step(xa, xa, t=601.0, reps=2, guidance=7.5, fuser_scale=1.0, sd_conv=False, noise=n, **k)
            assert torch.equal(xa, x2)
        # what it refuses, before anything is launched: a batch that does not match the conditioning, a tensor of another shape
        with pytest.raises(ValueError):
            eng.ddim_step(x[:1], x[:1], t=601.0, reps=1, guidance=7.5, fuser_scale=1.0, sd_conv=False, **kw)
        with pytest.raises(_lib.HipLibraryError):
            eng.ddim_step(x, x, t=601.0, reps=2, guidance=7.5, fuser_scale=1.0, sd_conv=False, noise=noise[:1], **kw)
        a = _lib.DdimStepArgs()
        a.x, a.x_out, a.reps = x.data_ptr(), x.data_ptr(), 3
        assert _lib.lib().gl_ddim_step(eng.handle, __import__("ctypes").byref(a), None) != 0
        a.x, a.reps = None, 2
        assert _lib.lib().gl_ddim_step(eng.handle, __import__("ctypes").byref(a), None) != 0
    finally:
        eng.use_graphs = True


# ------------------------------------------------------------------------------------------- the reference's runs through HIP
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_ddim_sampler_matches_reference_golden(case, strict):
    g = np.load(os.path.join(GOLD, case["name"] + ".npz"))
    inp = {a: T(v) for a, v in dc.case_inputs(case).items()}
    model = get_model(case["unet"], strict)
    draws = dc.unpack_draws(g)
    fake, state = dc.replayer(draws)
    out = run_ddim(model, case, inp, fake)
    assert state["n"] == len(draws), "the sampler drew as often as the reference, in its order and shapes"
    assert torch.isfinite(out).all()
    r_ddim, r_plms = rel_l2(out, T(g["out"])), plms_error(case["unet"], strict)
    _parity(case["name"], "strict" if strict else "default", r_ddim, r_plms)
    assert r_ddim < 2 * r_plms, (r_ddim, r_plms)


RECT_MASK = dict(name="ddim_rel_cfg_rect_mask", unet="rel", B=2, h=8, w=16, S=6, discretize="uniform", eta=1.0, guidance=7.5,
                 alpha_type=[0.3, 0.0, 0.7], mask=True)
REL_CFG = dict(name="ddim_rel_cfg", unet="rel", B=2, h=16, w=16, S=10, discretize="uniform", eta=0.5, guidance=7.5, alpha_type=[0.3, 0.0, 0.7],
               mask=False)


@pytest.mark.parametrize("case", [REL_CFG, RECT_MASK], ids=["square", "rect_mask_eta1"])
def test_relation_unet_with_guidance_matches_the_restated_loop(case):
    """classifier-free guidance on the relation UNet, which the reference's DDIM cannot run: against tests/ddim_ref.py driven by the
    oracle's eps function (fp32, CPU) with the same draws; the bound by the rule of the golden test"""
    if case["mask"]:
        inp = {k: T(v) for k, v in recipe.synth_inputs(TINY, case["B"], (case["h"], case["w"]), n_boxes=4, n_rel=3, seed=4321).items()}
        inp.update({k: T(v) for k, v in dc.mask_inputs(case["h"], case["w"]).items()})
    else:
        inp = {a: T(v) for a, v in dc.case_inputs(case).items()}
    model = get_model("rel")
    rec_fn, rec = dc.recorder(case["name"] + ".noise")
    out = run_ddim(model, case, inp, rec_fn)
    steps = 7 if case["mask"] else 10
    assert [tuple(a.shape) for a in rec] == ([tuple(inp["x0"].shape), tuple(inp["x"].shape)] * steps if case["mask"] else [tuple(inp["x"].shape)] * steps)
    sched = host.make_ddim_schedule(case["S"], host.alphas_cumprod(), case["discretize"], case["eta"])
    fake, state = dc.replayer(rec)
    with torch.no_grad(), dc.patched_randn_like(fake):
        ref = ddim_ref.ddim_sample(tog.make_eps_fn(case, inp, tog.tiny_sd(), TINY), inp["x"], sched, case["alpha_type"], mask=inp.get("mask"),
                                   x0=inp.get("x0"))
    assert state["n"] == len(rec) and torch.isfinite(out).all()
    r_ddim, r_plms = rel_l2(out, ref), plms_error("rel", False)
    _parity(case["name"], "default", r_ddim, r_plms)
    assert r_ddim < 2 * r_plms, (r_ddim, r_plms)


# ------------------------------------------------------------------------------------------- determinism
def test_eta0_is_deterministic_and_eta1_follows_its_draws():
    model = get_model("norel")
    c0, c1 = dc.by_name("ddim_norel_eta0"), dc.by_name("ddim_norel_eta1")
    inp = {a: T(v) for a, v in dc.case_inputs(c0).items()}
    torch.manual_seed(1)
    a = run_ddim(model, c0, inp).clone()
    torch.manual_seed(2)
    b = run_ddim(model, c0, inp).clone()
    assert torch.equal(a, b), "eta 0 is bit-equal from call to call, whatever the torch seed"
    draws = dc.unpack_draws(np.load(os.path.join(GOLD, "ddim_norel_eta1.npz")))
    e1 = run_ddim(model, c1, inp, dc.replayer(draws)[0]).clone()
    e2 = run_ddim(model, c1, inp, dc.replayer(draws)[0]).clone()
    assert torch.equal(e1, e2), "eta 1 with the same draws is bit-equal"
    e3 = run_ddim(model, c1, inp, dc.replayer(draws[::-1])[0])
    assert rel_l2(e3, e1) > 0.1 and rel_l2(e1, a) > 0.1, "other draws, or eta 0, give another latent"


# ------------------------------------------------------------------------------------------- the public switch
LOC = [[0.10, 0.10, 0.50, 0.55], [0.55, 0.20, 0.90, 0.70]]


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ckpt_ddim") / "tiny_gligen_text.pth")
    stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)      # 16 x 16 latents <-> 32 x 32 images
    stubs.install_fake_sng_parser()
    return p, itf.load_all_models(p, DEV), stubs.toy_clip().to(DEV), stubs.ToyProcessor()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_public_switch_run_one_image_and_gligen_inference(loaded):
    p, am, clip, proc = loaded
    model = am[0]
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5])
    noise = T(recipe.normal("gpuddim.noise", (2, 4, 16, 16), 9))
    base = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)

    def run(**more):
        model.first_conv_type = "GLIGEN"
        torch.manual_seed(7)
        return itf.run_one_image(am, dict(base, **more), dict(meta), noise.clone().to(DEV), clip, proc, device=DEV)
    today = run()
    assert _same(today, run(sampler="plms")), 'sampler = "plms" is the default path, byte for byte'
    d = run(sampler="ddim", ddim_eta=0.5)
    assert len(d) == 2 and all(im.size == (32, 32) and im.mode == "RGB" for im in d)
    assert all(np.asarray(im).std() > 0 for im in d) and not _same(d, today)
    assert _same(d, run(sampler="ddim", ddim_eta=0.5)), "the same seed gives the same images"
    assert not _same(d, run(sampler="ddim")), "eta changes the images"
    assert _same(today, run()), "the switch is per call: the next call without it runs PLMS"
    assert len(run(sampler="ddim", ddim_eta=0.5, ddim_discretize="quad")) == 2
    with pytest.raises(ValueError, match="plms"):
        run(ddim_eta=0.5)
    gi._MODELS[p] = am
    try:
        cfg = dict(batch_size=1, guidance_scale=7.5, no_plms=False, device=DEV, steps=4)
        m1 = dict(ckpt=p, prompt=meta["prompt"], phrases=meta["phrases"], locations=LOC)

        def grun(**more):
            torch.manual_seed(7)
            return gi.run(m1, dict(cfg, **more), starting_noise=noise[:1].clone().to(DEV), clip_model=clip, clip_processor=proc)
        a, b = grun(), grun(sampler="ddim", ddim_eta=0.5)
        assert len(b) == 1 and b[0].size == (32, 32) and not _same(a, b)
        assert _same(a, grun(sampler="plms")) and _same(b, grun(sampler="ddim", ddim_eta=0.5))
        with pytest.raises(NotImplementedError, match="sampler"):
            grun(no_plms=True)
    finally:
        gi._MODELS.pop(p, None)
