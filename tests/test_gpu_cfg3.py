"""Separate text and layout guidance scales (three-branch CFG) on the GPU: gl_cfg3_combine against the torch fp32 expression (bitwise) and
against gl_cfg_combine at equal scales (the derived rounding bound), the thirds of a reps = 3 forward against B-sized forwards,
``cfg3_eval`` against its two parts (bitwise), the three samplers against a loop written here from ``engine.forward``, the combine ops
and the op-level updates (bitwise, the draws replayed), what the scale means, and the public entries on synthetic checkpoints.

The models and helpers are test_gpu_ddim's: one set of TINY engines serves the sampler test files."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import cfg3_ref as c3
import ddim_cases as dc
import stubs
import test_gpu_ddim as tgd
from layoutllm_t2i_amd import _lib, host, ops, recipe
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.model import LatentDiffusion
from layoutllm_t2i_amd.sampler import DDIMSampler, DPMSolverSampler, PLMSSampler

DEV = "cuda:0"
T = torch.from_numpy
KEY = "layout_guidance_scale"
rel_l2 = tgd.rel_l2


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


# ------------------------------------------------------------------------------------------- 1. the kernel
# [1, 4, 8, 8] (256) and [2, 4, 8, 16] (1024: more than one block of float4s) take the float4 path; [1, 3, 5, 7] (105) the scalar one;
# "off": 256 elements whose eps3b starts one float behind a 16-byte boundary -- an aligned n on the scalar path
KSHAPES = [((1, 4, 8, 8), False), ((2, 4, 8, 16), False), ((1, 3, 5, 7), False), ((1, 4, 8, 8), True)]
SCALES = [(7.5, 12.0), (7.5, 0.0), (1.0, 3.0)]


def _eps3(shape, off):
    tag = "cfg3.k." + "x".join(map(str, shape))
    n = int(np.prod(shape))
    flat = T(recipe.normal(tag, (3 * n + 4,), 3)).to(DEV)
    eps = flat[1:1 + 3 * n] if off else flat[4:4 + 3 * n].clone()
    eps = eps.view((3 * shape[0],) + tuple(shape[1:]))
    assert eps.data_ptr() % 16 == (4 if off else 0) and eps.is_contiguous()
    return eps


@pytest.mark.parametrize("scales", SCALES, ids=[f"{a}-{b}" for a, b in SCALES])
@pytest.mark.parametrize("shape,off", KSHAPES, ids=["x".join(map(str, s)) + ("-off" if o else "") for s, o in KSHAPES])
def test_cfg3_combine_is_bitwise_the_torch_expression(shape, off, scales):
    s_t, s_l = scales
    eps = _eps3(shape, off)
    before = eps.clone()
    ref = c3.torch_combine3(eps, s_t, s_l)
    out = torch.full(shape, float("nan"), device=DEV)
    got = ops.cfg3_combine(eps, s_t, s_l, out)
    assert got is out and torch.isfinite(ref).all() and torch.equal(out, ref), float((out - ref).abs().max())
    assert torch.equal(eps, before)
    e_c, e_t, e_u = eps.chunk(3, 0)
    if s_l == 0:
        assert torch.equal(out, e_u + s_t * (e_t - e_u)), "the conditional third is weighted by zero"
    # equal scales: gl_cfg_combine on [cond ; uncond] up to the rounding of the two expressions (tests/cfg3_ref.py derives the bound)
    two = ops.cfg_combine(torch.cat([e_c, e_u], 0).contiguous(), s_t, torch.empty(shape, device=DEV))
    same = ops.cfg3_combine(eps, s_t, s_t, torch.empty(shape, device=DEV))
    bound = c3.same_scale_bound(*(t.double().cpu().numpy() for t in (e_c, e_t, e_u)), s_t)
    err = (same.double() - two.double()).abs().cpu().numpy()
    print(f"[cfg3_kernel] {shape} s = {s_t}: max |cfg3(s, s) - cfg2(s)| = {err.max():.3e}, max of the bound {bound.max():.3e}, worst ratio {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert not torch.equal(same, out) or s_t == s_l


def test_cfg3_combine_refuses_bad_operands():
    eps, out = torch.zeros(6, 4, 8, 8, device=DEV), torch.zeros(2, 4, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.cfg3_combine(eps[:4], 1.0, 1.0, out)                 # 2n, not 3n
    with pytest.raises(ValueError):
        ops.cfg3_combine(eps[:, :, ::2], 1.0, 1.0, out[:, :, ::2])
    with pytest.raises(_lib.HipLibraryError):
        ops.cfg3_combine(eps.cpu(), 1.0, 1.0, out)
    lib = _lib.lib()
    assert lib.gl_cfg3_combine(eps.data_ptr(), 1.0, 1.0, 0, out.data_ptr(), None) == -1
    assert lib.gl_cfg3_combine(None, 1.0, 1.0, 512, out.data_ptr(), None) == -1
    assert lib.gl_cfg3_combine(eps.data_ptr(), 1.0, 1.0, 512, None, None) == -1


# ------------------------------------------------------------------------------------------- 2. the thirds of a reps = 3 forward
B = 2


def _inputs(cfg, b, hw, seed=77):
    return {k: T(v) for k, v in recipe.synth_inputs(cfg, b, hw, n_boxes=4, n_rel=3, seed=seed).items()}


def _parts(model, inp):
    """the conditioning of the three branches, B-sized each: (context, relations, boxes, masks, embeddings)"""
    z = torch.zeros_like
    rel = inp["relations"] if model.cfg.relation else None
    real = (inp["boxes"], inp["masks"], inp["positive_embeddings"])
    null = tuple(z(t) for t in real)
    return dict(cond=(inp["context"], rel, *real), text=(inp["context"], rel, *null), uncond=(inp["uc"], rel, *null))


def _set(model, inp, names):
    parts = _parts(model, inp)
    cols = list(zip(*[parts[n] for n in names]))
    cat = [None if c[0] is None else torch.cat(list(c), 0) for c in cols]
    h, w = (int(v) for v in inp["x"].shape[-2:])
    model.engine.set_conditioning(*cat, h if h == w else (h, w))


THREE, TWO = ("cond", "text", "uncond"), ("cond", "uncond")


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("hw", [(8, 8), (8, 16)], ids=["8x8", "8x16"])
@pytest.mark.parametrize("unet", ["rel", "norel"])
def test_each_third_equals_its_own_forward(unet, hw, strict):
    model = tgd.get_model(unet, strict)
    eng = model.engine
    inp = _inputs(model.cfg, B, hw)
    x = inp["x"].to(DEV).contiguous()
    t, fuser = 601.0, 1.0
    single = {}
    for name in THREE:
        _set(model, inp, (name,))
        single[name] = eng.forward(x, t, fuser, False, 1).clone()
    _set(model, inp, TWO)
    e2 = eng.forward(x, t, fuser, False, 2).clone()
    r2 = max(rel_l2(e2[:B], single["cond"]), rel_l2(e2[B:], single["uncond"]))
    bound = max(1e-6, 2 * r2)
    _set(model, inp, THREE)
    try:
        eng.use_graphs = False
        eager = eng.forward(x, t, fuser, False, 3).clone()
        eng.use_graphs = True
        first = eng.forward(x, t, fuser, False, 3).clone()          # captures
        replay = eng.forward(x, t, fuser, False, 3).clone()         # replays
    finally:
        eng.use_graphs = True
    assert tuple(eager.shape) == (3 * B, 4) + hw and torch.isfinite(eager).all()
    assert torch.equal(first, eager) and torch.equal(replay, eager), "graph replay equals eager, bitwise"
    r3 = [rel_l2(eager[i * B:(i + 1) * B], single[name]) for i, name in enumerate(THREE)]
    print(f"[cfg3_thirds] {unet:5s} {hw[0]}x{hw[1]} {'strict' if strict else 'default':7s} rel_l2 of the thirds {r3[0]:.2e} {r3[1]:.2e} {r3[2]:.2e}   "
          f"halves of reps = 2: {r2:.2e}   bound {bound:.2e}")
    assert max(r3) <= bound, (r3, bound)
    # the thirds are three different problems
    assert rel_l2(single["cond"], single["text"]) > 1e-3 and rel_l2(single["text"], single["uncond"]) > 1e-3


# ------------------------------------------------------------------------------------------- 3. cfg3_eval == forward + combine
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("unet", ["rel", "norel"])
def test_cfg3_eval_equals_forward_plus_combine(unet, graphs):
    assert _lib.lib().gl_sizeof_cfg3_eval_args() == ctypes.sizeof(_lib.Cfg3EvalArgs)
    model = tgd.get_model(unet)
    eng = model.engine
    inp = _inputs(model.cfg, B, (8, 16), seed=21)
    x = inp["x"].to(DEV).contiguous()
    _set(model, inp, THREE)
    eng.use_graphs = graphs
    try:
        for fuser, sd in ((1.0, False), (0.0, True), (0.3, False)):
            e = torch.full_like(x, float("nan"))
            got = eng.cfg3_eval(x, e, t=481.0, fuser_scale=fuser, sd_conv=sd, s_text=7.5, s_layout=12.0)
            eps = eng.forward(x, 481.0, fuser, sd, 3).clone()
            want = ops.cfg3_combine(eps, 7.5, 12.0, torch.empty_like(x))
            assert got is e and torch.isfinite(want).all() and torch.equal(e, want), (fuser, sd)
        # what it refuses, before anything is launched
        with pytest.raises(_lib.HipLibraryError):
            eng.cfg3_eval(x, None, t=481.0, fuser_scale=1.0, sd_conv=False, s_text=7.5, s_layout=12.0)
        with pytest.raises(_lib.HipLibraryError):
            eng.cfg3_eval(x, torch.empty_like(x)[:1], t=481.0, fuser_scale=1.0, sd_conv=False, s_text=7.5, s_layout=12.0)
        a = _lib.Cfg3EvalArgs()
        a.x, a.e_out, a.t, a.reps, a.fuser_scale, a.s_text, a.s_layout = x.data_ptr(), None, 481.0, 3, 1.0, 7.5, 12.0
        assert _lib.lib().gl_cfg3_eval(eng.handle, ctypes.byref(a), None) == -1                        # NULL e_out
        keep = torch.empty_like(x)
        a.e_out, a.reps = keep.data_ptr(), 2
        assert _lib.lib().gl_cfg3_eval(eng.handle, ctypes.byref(a), None) == -1                        # its reps is 3
        # the existing steps keep refusing reps = 3 on the 3B batch
        d = _lib.DdimStepArgs()
        d.x, d.x_out, d.reps = x.data_ptr(), keep.data_ptr(), 3
        assert _lib.lib().gl_ddim_step(eng.handle, ctypes.byref(d), None) == -1
        # a 2B conditioning batch
        _set(model, inp, TWO)
        with pytest.raises(ValueError):
            eng.cfg3_eval(x, torch.empty_like(x), t=481.0, fuser_scale=1.0, sd_conv=False, s_text=7.5, s_layout=12.0)
        a.reps = 3
        assert _lib.lib().gl_cfg3_eval(eng.handle, ctypes.byref(a), None) == -1
        assert "multiple of 3" in _lib.last_error(eng.handle)
    finally:
        eng.use_graphs = True


def test_cfg3_eval_refuses_the_sd_conv_without_sd_weights():
    import dataclasses
    from layoutllm_t2i_amd.model import GroundingNetInput, UNetModel
    model = UNetModel(dataclasses.replace(TINY), recipe.state_dict(TINY, 0), device=DEV, sd_first_conv=None)
    model.grounding_tokenizer_input = GroundingNetInput()
    inp = _inputs(TINY, 1, (8, 8))
    x = inp["x"].to(DEV).contiguous()
    _set(model, inp, THREE)
    with pytest.raises(RuntimeError, match="SD first-conv"):
        model.engine.cfg3_eval(x, torch.empty_like(x), t=481.0, fuser_scale=0.0, sd_conv=True, s_text=7.5, s_layout=12.0)
    a = _lib.Cfg3EvalArgs()
    keep = torch.empty_like(x)
    a.x, a.e_out, a.t, a.reps, a.sd_conv = x.data_ptr(), keep.data_ptr(), 481.0, 3, 1
    assert _lib.lib().gl_cfg3_eval(model.engine.handle, ctypes.byref(a), None) == -1
    del model
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- 4. the samplers against a loop written here
S, G, SL, ETA = 6, 7.5, 12.0, 0.5
ALPHA = {"rel": [0.3, 0.0, 0.7], "norel": [0.5, 0.0, 0.5]}
ACP = host.alphas_cumprod()
CLASSES = {"plms": (PLMSSampler, {}), "ddim": (DDIMSampler, dict(eta=ETA)), "dpmpp_2m": (DPMSolverSampler, {})}


def run_sampler(model, name, inp, alpha_type, layout, randn_like, guidance=G, steps=S):
    cls, kw = CLASSES[name]
    model.first_conv_type = "GLIGEN"
    s = cls(LatentDiffusion(device=DEV), model, **kw, **tgd._callbacks(alpha_type))
    with dc.patched_randn_like(randn_like):
        out = s.sample_layout(S=steps, shape=tuple(inp["x"].shape), input=tgd._input(model, inp), uc=inp["uc"], guidance_scale=guidance,
                              layout_guidance_scale=layout, mask=inp.get("mask"), x0=inp.get("x0")).clone()
    model.first_conv_type = "GLIGEN"
    return out


def manual_loop(model, name, inp, alpha_type, layout, randn_like):
    """the three-branch sampler restated: per step the blend, the evaluation in the form the rule of the steps asks for (3B + cfg3_combine, or
    2B + cfg_combine where the step cannot see the grounding), the sampler's op-level update on the B-sized guided eps"""
    eng = model.engine
    sched = {"plms": lambda: host.make_schedule(S, ACP), "ddim": lambda: host.make_ddim_schedule(S, ACP, "uniform", ETA),
             "dpmpp_2m": lambda: host.make_dpm_schedule(S, ACP, "logsnr")}[name]()
    ts = [int(t) for t in np.flip(sched["ddim_timesteps"])]
    n = len(ts)
    alphas = host.alpha_generator(n, alpha_type)
    ld = LatentDiffusion(device=DEV)
    sac, s1ac = ld.sqrt_alphas_cumprod.cpu().numpy(), ld.sqrt_one_minus_alphas_cumprod.cpu().numpy()
    x = inp["x"].to(DEV, torch.float32).contiguous().clone()
    state = dict(form=None, sd=False, forms=[])

    def guided(x_eval, t, alpha):
        want = THREE if c3.needs_text_branch(model.cfg.relation, alpha) else TWO
        if want != state["form"]:
            _set(model, inp, want)
            state["form"] = want
        state["forms"].append(len(want))
        eps = eng.forward(x_eval, float(t), alpha, state["sd"], len(want))
        e = torch.empty_like(x_eval)
        return ops.cfg3_combine(eps, G, layout, e) if want is THREE else ops.cfg_combine(eps, G, e)

    old, prev = [], None
    hist = torch.empty_like(x)
    with dc.patched_randn_like(randn_like):
        for i, t in enumerate(ts):
            index, alpha = n - i - 1, alphas[i]
            state["sd"] = state["sd"] or alpha == 0
            if "mask" in inp:
                noise = torch.randn_like(inp["x0"]).to(DEV, torch.float32).contiguous()
                ops.latent_blend(x, inp["x0"].to(DEV).contiguous(), noise, inp["mask"].to(DEV).contiguous(), float(sac[t]), float(s1ac[t]))
            if name == "plms":
                coef = host.step_coefs(sched, index)
                torch.randn_like(x)
                e_t = guided(x, t, alpha)
                if not old:
                    x_mid = ops.plms_update(x, e_t, [], (1.0,), 1.0, *coef, torch.empty_like(x))
                    torch.randn_like(x)
                    e_next = guided(x_mid, ts[min(i + 1, n - 1)], alpha)
                    coefs, div = host.PLMS_COEFS[0]
                    ops.plms_update(x, e_t, [e_next], coefs, div, *coef, x)
                else:
                    coefs, div = host.PLMS_COEFS[min(len(old), 3)]
                    ops.plms_update(x, e_t, old[::-1][:len(coefs) - 1], coefs, div, *coef, x)
                old.append(e_t)
                if len(old) > 3:
                    old.pop(0)
            elif name == "ddim":
                sq_at, s1m, sq_ap, dirc, sigma = host.ddim_step_coefs(sched, index)
                noise = torch.randn_like(x)
                e = guided(x, t, alpha)
                ops.ddim_update(e, x, x, sqrt_at=sq_at, s1m=s1m, sqrt_aprev=sq_ap, dir_coef=dirc, sigma=sigma, noise=noise if sigma != 0 else None)
            else:
                sq_at, s1m, c_x, c_d, w1, w0 = host.dpm_step_coefs(sched, index, prev, 2)
                e = guided(x, t, alpha)
                ops.dpmpp_update(e, x, x, hist, sqrt_at=sq_at, s1m=s1m, c_x=c_x, c_d=c_d, w1=w1, w0=w0, x0_old=hist if w0 != 0 else None)
                prev = index
    return x, state["forms"]


def _check_sampler(unet, name, inp):
    model = tgd.get_model(unet)
    rec_fn, rec = dc.recorder(f"cfg3.{unet}.{name}.noise")
    out = run_sampler(model, name, inp, ALPHA[unet], SL, rec_fn)
    replay, st = dc.replayer(rec)
    want, forms = manual_loop(model, name, inp, ALPHA[unet], SL, replay)
    assert st["n"] == len(rec), "the sampler drew exactly what the loop draws, in its order"
    assert torch.isfinite(want).all() and torch.equal(out, want), float((out - want).abs().max())
    if unet == "rel":
        assert set(forms) == {3}
    else:
        k = forms.index(2)
        assert 0 < k < len(forms) and set(forms[:k]) == {3} and set(forms[k:]) == {2}, "one switch per image"
    # the layout scale matters, and it is not the text scale in disguise
    plain = run_sampler(model, name, inp, ALPHA[unet], None, dc.replayer(rec)[0])
    assert rel_l2(out, plain) > 1e-3
    return out


@pytest.mark.parametrize("name", list(CLASSES))
@pytest.mark.parametrize("unet", ["rel", "norel"])
def test_sampler_equals_the_restated_loop(unet, name):
    model = tgd.get_model(unet)
    _check_sampler(unet, name, _inputs(model.cfg, 1, (8, 8), seed=31))


def test_masked_rectangular_dpm_sampler_equals_the_restated_loop():
    for unet in ("rel", "norel"):
        model = tgd.get_model(unet)
        inp = _inputs(model.cfg, 1, (8, 16), seed=32)
        inp.update({k: T(v) for k, v in dc.mask_inputs(8, 16).items()})
        _check_sampler(unet, "dpmpp_2m", inp)


# ------------------------------------------------------------------------------------------- 5. what the scale means
@pytest.mark.parametrize("unet", ["rel", "norel"])
def test_layout_scale_semantics(unet):
    model = tgd.get_model(unet)
    inp = _inputs(model.cfg, 1, (8, 8), seed=41)
    moved = dict(inp, boxes=inp["boxes"] * 0.5, positive_embeddings=inp["positive_embeddings"] * -1.0)
    assert not torch.equal(moved["boxes"], inp["boxes"])
    draw = lambda: dc.recorder("cfg3.sem.noise")[0]
    a = run_sampler(model, "plms", inp, ALPHA[unet], 0.0, draw())
    b = run_sampler(model, "plms", moved, ALPHA[unet], 0.0, draw())
    assert torch.isfinite(a).all() and torch.equal(a, b), "layout scale 0: the boxes do not matter"
    c = run_sampler(model, "plms", moved, ALPHA[unet], 7.5, draw())
    assert not torch.equal(c, run_sampler(model, "plms", inp, ALPHA[unet], 7.5, draw())), "(with a scale they do)"
    lo, hi = run_sampler(model, "plms", inp, ALPHA[unet], 7.5, draw()), run_sampler(model, "plms", inp, ALPHA[unet], 15.0, draw())
    r = rel_l2(hi, lo)
    print(f"[cfg3_semantics] {unet}: rel_l2 between layout scales 7.5 and 15 = {r:.3e}")
    assert r > 1e-3
    # equal scales: today's guidance up to rounding (informational; the two runs differ in the batch form of every three-branch step)
    model.first_conv_type = "GLIGEN"
    s = PLMSSampler(LatentDiffusion(device=DEV), model, **tgd._callbacks(ALPHA[unet]))
    with dc.patched_randn_like(draw()):
        today = s.sample(S=S, shape=tuple(inp["x"].shape), input=tgd._input(model, inp), uc=inp["uc"], guidance_scale=G).clone()
    model.first_conv_type = "GLIGEN"
    print(f"[cfg3_semantics] {unet}: rel_l2 between layout scale == guidance scale and the two-branch run = {rel_l2(lo, today):.3e}")
    # guidance_scale 1 with a layout scale still runs three branches
    one = run_sampler(model, "plms", inp, ALPHA[unet], 7.5, draw(), guidance=1)
    assert torch.isfinite(one).all() and rel_l2(one, lo) > 1e-3


# ------------------------------------------------------------------------------------------- 6. the public entries
LOC = [[0.10, 0.10, 0.50, 0.55], [0.55, 0.20, 0.90, 0.70]]
_same = tgd._same


def _images_ok(ims, n):
    return len(ims) == n and all(im.size == (32, 32) and im.mode == "RGB" and np.asarray(im).std() > 0 for im in ims)


@pytest.fixture(scope="module")
def text_ckpt(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ckpt_cfg3") / "tiny_gligen_text.pth")
    stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)      # 16 x 16 latents <-> 32 x 32 images
    stubs.install_fake_sng_parser()
    return p, itf.load_all_models(p, DEV), stubs.toy_clip().to(DEV), stubs.ToyProcessor()


META = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5])
BASE = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)
NOISE = T(recipe.normal("gpucfg3.noise", (2, 4, 16, 16), 9))


def _run_text(am, clip, proc, **more):
    am[0].first_conv_type = "GLIGEN"
    return itf.run_one_image(am, dict(BASE, **more), dict(META), NOISE.clone().to(DEV), clip, proc, device=DEV)


def test_text_checkpoint_keeps_no_state_of_the_key(text_ckpt):
    p, am, clip, proc = text_ckpt
    keyed = _run_text(am, clip, proc, **{KEY: 12})
    assert _images_ok(keyed, 2)
    after = _run_text(am, clip, proc)                                  # the cached config still holds the key: the call decides
    fresh = _run_text(itf.load_all_models(p, DEV), clip, proc)         # a handle that has never seen the key
    assert _same(after, fresh), "the feature leaves no state behind on the engine"
    assert not _same(keyed, after)


def test_text_checkpoint_takes_the_key_under_every_sampler(text_ckpt):
    p, am, clip, proc = text_ckpt
    keyed = _run_text(am, clip, proc, **{KEY: 12})
    assert _same(keyed, _run_text(am, clip, proc, **{KEY: 12.0})) and not _same(keyed, _run_text(am, clip, proc, **{KEY: 3}))
    assert _images_ok(_run_text(am, clip, proc, sampler="dpmpp_2m", **{KEY: 12}), 2)
    assert _images_ok(_run_text(am, clip, proc, sampler="ddim", ddim_eta=0.5, **{KEY: 12}), 2)
    am[0].first_conv_type = "GLIGEN"
    bmeta = dict(prompts=[META["prompt"]] * 2, phrases=[META["phrases"]] * 2, locations=[LOC] * 2, alpha_type=META["alpha_type"])
    assert _images_ok(itf.run_batch_images(am, dict(BASE, **{KEY: 12}), dict(bmeta), NOISE.clone().to(DEV), clip, proc, device=DEV), 2)
    with pytest.raises(ValueError, match=KEY):
        _run_text(am, clip, proc, **{KEY: -1})


def test_keypoint_checkpoint_takes_the_key(tmp_path):
    import test_gpu_kp as tkp
    p = str(tmp_path / "tiny_gligen_keypoint.pth")
    tkp._write_kp_checkpoint(p, 3)
    am = itf.load_all_models(p, DEV)
    locations = np.load(os.path.join(tgd.GOLD, "kp_prepare_batch.npz"))["locations"].tolist()
    meta = dict(prompt="A young man and a small boy are talking", locations=locations, alpha_type=[0.5, 0.0, 0.5])
    noise = T(recipe.normal("gpucfg3.kp.noise", (2, 4, 16, 16), 9))
    args = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)

    def run(**more):
        am[0].first_conv_type = "GLIGEN"
        return itf.run_one_image(am, dict(args, **more), dict(meta), noise.clone().to(DEV), None, None, device=DEV)
    plain, keyed = run(), run(**{KEY: 12})
    assert _images_ok(keyed, 2) and not _same(plain, keyed) and _same(plain, run())
    am[0].first_conv_type = "GLIGEN"
    both = itf.run_batch_images(am, dict(args, **{KEY: 12}), dict(prompts=[meta["prompt"]] * 2, locations=[locations] * 2, alpha_type=meta["alpha_type"]),
                                noise.clone().to(DEV), None, None, device=DEV)
    assert _images_ok(both, 2)


def test_canny_checkpoint_refuses_the_key_before_any_kernel(tmp_path):
    import sp_cases as sc
    import test_gpu_sp as tsp
    from PIL import Image
    p = str(tmp_path / "tiny_gligen_canny.pth")
    tsp._write_canny_checkpoint(p)
    am = itf.load_all_models(p, DEV)
    img = str(tmp_path / "edges.png")
    Image.fromarray(sc.test_image()).save(img)
    launches = am[0].engine.num_launches()
    cond = am[0].engine.cond
    with pytest.raises(ValueError, match=KEY):
        itf.run_one_image(am, {"batch_size": 2, "no_plms": False, "guidance_scale": 7.5, "steps": 4, KEY: 3.0},
                          dict(prompt="a house by a lake", canny_image=img, alpha_type=[0.5, 0.0, 0.5]), torch.zeros(2, 4, 16, 16, device=DEV), None, None,
                          device=DEV)
    assert am[0].engine.cond is cond and am[0].engine.num_launches() == launches and KEY not in am[4]
