"""The DPM-Solver++(2M) sampler on the GPU: gl_dpmpp_update against the torch fp32 expression (bitwise), gl_dpmpp_step against its two parts
(bitwise), ``DPMSolverSampler`` against the float64 loop of tests/dpmpp_ref.py driven by the oracle UNet in default and strict mode,
determinism, and the public switch on a synthetic checkpoint.

The sampler's bound is relative, as in tests/test_gpu_ddim.py and for the same reason (the sampler adds no error source beyond the UNet's):
in the same run the existing ``PLMSSampler`` is measured on its golden of the same model and mode, and this sampler must stay below twice
that error.  Both values are printed (``[dpmpp_parity] ...``; profiles/dpmpp_parity.txt holds a recorded run).  The models, the PLMS
yardstick and the helpers are test_gpu_ddim's: one set of engines serves both files."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import ddim_cases as dc
import dpmpp_ref as dr
import golden_cases as gc
import norel_cases as nc
import norel_ref
import stubs
import test_gpu_ddim as tgd
import test_oracle_golden as tog
from layoutllm_t2i_amd import _lib, host, ops, recipe, txt2img
from layoutllm_t2i_amd import gligen_inference as gi
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.model import LatentDiffusion
from layoutllm_t2i_amd.sampler import DPMSolverSampler
from oracle import plms_ref

DEV = "cuda:0"
T = torch.from_numpy
ACP = host.alphas_cumprod()
NAMES = ("sqrt_at", "s1m", "c_x", "c_d", "w1", "w0")


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


# ------------------------------------------------------------------------------------------- 6. the kernel, bit for bit
SCHED10 = host.make_dpm_schedule(10, ACP)
COEFS2 = host.dpm_step_coefs(SCHED10, 5, 6, 2)        # a second-order step of a real S = 10 schedule: w0 != 0
COEFS1 = host.dpm_step_coefs(SCHED10, 9, None, 2)     # its first step: (w1, w0) = (1, 0)
# [1] and [1, 3, 7, 13] (273 elements: two blocks and a tail) take the scalar path; [1, 4, 3, 5] (60) and [2, 4, 16, 16] the float4 path
SHAPES = [(1,), (1, 4, 3, 5), (2, 4, 16, 16), (1, 3, 7, 13)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("reps", [1, 2])
def test_dpmpp_update_is_bitwise_the_torch_expression(shape, reps):
    assert COEFS2[5] != 0 and COEFS1[4:] == (1.0, 0.0)
    tag = "dpmpp.k." + "x".join(map(str, shape))
    x = T(recipe.normal(tag + ".x", shape, 3)).to(DEV)
    eps = T(recipe.normal(tag + ".eps", (reps * shape[0],) + tuple(shape[1:]), 3)).to(DEV)
    old = T(recipe.normal(tag + ".old", shape, 3)).to(DEV)
    for second in (False, True):
        coefs = COEFS2 if second else COEFS1
        kw = dict(zip(NAMES, coefs), guidance=7.5)
        ref, ref_p = dr.torch_update(eps, x, old if second else None, reps, 7.5, coefs)
        assert torch.isfinite(ref).all() and not torch.equal(ref, ref_p)
        for x_in_place in (False, True):
            for hist_in_place in ((False, True) if second else (False,)):
                xin, oin = x.clone(), old.clone()
                out = xin if x_in_place else torch.full_like(x, float("nan"))
                pred = oin if hist_in_place else torch.full_like(x, float("nan"))
                got = ops.dpmpp_update(eps, xin, out, pred, x0_old=oin if second else None, **kw)
                assert got is out and torch.equal(out, ref), (second, x_in_place, hist_in_place, float((out - ref).abs().max()))
                assert torch.equal(pred, ref_p)
                assert x_in_place or torch.equal(xin, x)
                assert hist_in_place or torch.equal(oin, old)
    # the history term is real: the second-order result is not the first-order one with the same scalars
    assert not torch.equal(dr.torch_update(eps, x, old, reps, 7.5, COEFS2)[0], dr.torch_update(eps, x, None, reps, 7.5, COEFS2)[0])


def test_dpmpp_update_on_unaligned_pointers_and_bad_arguments():
    """a 4-byte-aligned view takes the scalar path whatever n is; what the entry refuses"""
    base = {k: T(recipe.normal(f"dpmpp.k.un.{k}", (2 * 512 + 1,), 3)).to(DEV) for k in ("x", "eps", "old", "out", "pred")}
    x, old, out, pred = (base[k][1:257] for k in ("x", "old", "out", "pred"))
    eps = base["eps"][1:513]
    assert all(t.data_ptr() % 16 == 4 for t in (x, old, out, pred, eps))
    kw = dict(zip(NAMES, COEFS2))
    ops.dpmpp_update(eps, x, out, pred, x0_old=old, guidance=3.0, **kw)
    ref, ref_p = dr.torch_update(eps.reshape(2, 256), x.reshape(1, 256), old.reshape(1, 256), 2, 3.0, COEFS2)
    assert torch.equal(out, ref.reshape(-1)) and torch.equal(pred, ref_p.reshape(-1))
    for k in ("out", "pred"):
        orig = T(recipe.normal(f"dpmpp.k.un.{k}", (1025,), 3)).to(DEV)
        assert torch.equal(base[k][257:], orig[257:]) and torch.equal(base[k][:1], orig[:1]), "nothing written around the view"
    # in place on the unaligned views, history included
    xin, oin = base["x"].clone()[1:257], base["old"].clone()[1:257]
    ops.dpmpp_update(eps, xin, xin, oin, x0_old=oin, guidance=3.0, **kw)
    assert torch.equal(xin, ref.reshape(-1)) and torch.equal(oin, ref_p.reshape(-1))
    # only ONE unaligned pointer among aligned ones: still the scalar path, still the same bits
    xa, oa, outa, preda = (t.clone() for t in (x, old, out, pred))
    assert xa.data_ptr() % 16 == 0
    ops.dpmpp_update(eps, xa, outa, preda, x0_old=oa, guidance=3.0, **kw)
    assert torch.equal(outa, ref.reshape(-1)) and torch.equal(preda, ref_p.reshape(-1))
    with pytest.raises(ValueError):
        ops.dpmpp_update(base["eps"][:300], x, out, pred, **dict(zip(NAMES, COEFS1)))       # neither n nor 2n
    with pytest.raises(ValueError):
        ops.dpmpp_update(eps, x, base["out"][:100], pred, **dict(zip(NAMES, COEFS1)))
    with pytest.raises(ValueError):
        ops.dpmpp_update(eps, x, out, pred, **kw)                                           # w0 != 0 without x0_old
    with pytest.raises(ValueError):
        ops.dpmpp_update(eps, x, out, None, **dict(zip(NAMES, COEFS1)))                     # x0_out is required
    with pytest.raises(_lib.HipLibraryError):
        ops.dpmpp_update(eps.cpu(), x, out, pred, **dict(zip(NAMES, COEFS1)))
    lib = _lib.lib()
    p = dict(eps=eps.data_ptr(), x=x.data_ptr(), old=old.data_ptr(), out=out.data_ptr(), pred=pred.data_ptr())
    call = lambda eps, x, old, reps, w0, n, out, pred: lib.gl_dpmpp_update(eps, x, old, reps, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, w0, n, out, pred, None)
    assert call(p["eps"], p["x"], p["old"], 3, 0.0, 256, p["out"], p["pred"]) == -1
    assert call(None, p["x"], p["old"], 1, 0.0, 256, p["out"], p["pred"]) == -1
    assert call(p["eps"], p["x"], p["old"], 1, 0.0, 0, p["out"], p["pred"]) == -1
    assert call(p["eps"], p["x"], p["old"], 1, 0.0, 256, p["out"], None) == -1
    assert call(p["eps"], p["x"], None, 1, -0.5, 256, p["out"], p["pred"]) == -1


# ------------------------------------------------------------------------------------------- 7. fused step == its two parts
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_dpmpp_step_equals_forward_plus_update(graphs):
    assert _lib.lib().gl_sizeof_dpmpp_step_args() == ctypes.sizeof(_lib.DpmppStepArgs)
    model = tgd.get_model("rel")
    eng = model.engine
    inp = {k: T(v) for k, v in recipe.synth_inputs(TINY, 2, 16, n_boxes=4, n_rel=3, seed=21).items()}
    z, cat = torch.zeros_like, lambda p, q: torch.cat([p, q], 0)
    eng.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
                         cat(inp["masks"], z(inp["masks"])), cat(inp["positive_embeddings"], z(inp["positive_embeddings"])), 16)
    x = inp["x"].to(DEV).contiguous()
    old = T(recipe.normal("dpmpp.step.old", tuple(x.shape), 3)).to(DEV)
    base = dict(t=601.0, reps=2, guidance=7.5, sd_conv=False)
    eng.use_graphs = graphs
    try:
        for fuser in (1.0, 0.0):
            for second in (True, False):
                kw = dict(zip(NAMES, COEFS2 if second else COEFS1))
                h = old if second else None
                x_out, pred = torch.empty_like(x), torch.empty_like(x)
                eng.dpmpp_step(x, x_out, pred, fuser_scale=fuser, x0_old=h, **base, **kw)
                eps = eng.forward(x, 601.0, fuser, False, 2).clone()
                pred2 = torch.empty_like(x)
                x2 = ops.dpmpp_update(eps, x, torch.empty_like(x), pred2, x0_old=h, guidance=7.5, **kw)
                assert torch.isfinite(x2).all() and torch.equal(x_out, x2) and torch.equal(pred, pred2), (fuser, second)
                # the in-place form the sampler uses: the latent in place, ONE history buffer
                xa, ha = x.clone(), old.clone()
                eng.dpmpp_step(xa, xa, ha, fuser_scale=fuser, x0_old=ha if second else None, **base, **kw)
                assert torch.equal(xa, x2) and torch.equal(ha, pred2)
        # what it refuses, before anything is launched
        kw1 = dict(zip(NAMES, COEFS1))
        with pytest.raises(ValueError):
            eng.dpmpp_step(x[:1], x[:1], old[:1], fuser_scale=1.0, **dict(base, reps=1), **kw1)      # batch does not match the conditioning
        with pytest.raises(_lib.HipLibraryError):
            eng.dpmpp_step(x, x, old[:1], fuser_scale=1.0, **base, **kw1)
        with pytest.raises(ValueError):
            eng.dpmpp_step(x, x, old, fuser_scale=1.0, **base, **dict(zip(NAMES, COEFS2)))           # w0 != 0 without x0_old
        a = _lib.DpmppStepArgs()
        a.x, a.x_out, a.x0_out, a.reps, a.w1 = x.data_ptr(), x.data_ptr(), old.data_ptr(), 3, 1.0
        assert _lib.lib().gl_dpmpp_step(eng.handle, ctypes.byref(a), None) == -1
        a.reps, a.x0_out = 2, None
        assert _lib.lib().gl_dpmpp_step(eng.handle, ctypes.byref(a), None) == -1
        a.x0_out, a.w0 = old.data_ptr(), -0.5                                                        # no x0_old, but a history weight
        assert _lib.lib().gl_dpmpp_step(eng.handle, ctypes.byref(a), None) == -1
    finally:
        eng.use_graphs = True


# ------------------------------------------------------------------------------------------- 8. the sampler against the float64 loop
_COMMON = dict(B=2, h=16, w=16, guidance=7.5, alpha_type=[0.3, 0.0, 0.7], order=2, mask=False)
CASES = [
    dict(_COMMON, name="dpmpp_norel_logsnr", unet="norel", S=10, discretize="logsnr"),
    dict(_COMMON, name="dpmpp_norel_quad", unet="norel", S=6, discretize="quad"),
    dict(_COMMON, name="dpmpp_rel_logsnr", unet="rel", S=10, discretize="logsnr"),
    dict(_COMMON, name="dpmpp_rel_quad", unet="rel", S=6, discretize="quad"),
    # a rectangular latent, masked: x0 and mask of batch 1, the blend's draws recorded
    dict(_COMMON, name="dpmpp_rel_rect_mask", unet="rel", h=8, w=16, S=6, discretize="logsnr", mask=True),
]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    case = next(c for c in CASES if c["name"] == name)
    if case["mask"]:
        inp = {k: T(v) for k, v in recipe.synth_inputs(TINY, case["B"], (case["h"], case["w"]), n_boxes=4, n_rel=3, seed=4321).items()}
        inp.update({k: T(v) for k, v in dc.mask_inputs(case["h"], case["w"]).items()})
        return inp
    return {a: T(v) for a, v in (nc if case["unet"] == "norel" else gc).case_inputs(dc.plms_case(case)).items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 loop of tests/dpmpp_ref.py over the oracle UNet (fp32, CPU), once per case: both modes are measured against it"""
    case = next(c for c in CASES if c["name"] == name)
    inp = case_inputs(name)
    if case["unet"] == "norel":
        sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(nc.NR_TINY, 0).items()}
        fc = {a: T(v) for a, v in recipe.sd_first_conv(nc.NR_TINY, 0).items()}
        oracle_eps = norel_ref.make_eps_fn(sd, nc.NR_TINY, inp, case["guidance"], fc)
    else:
        oracle_eps = tog.make_eps_fn(case, inp, tog.tiny_sd(), TINY)
    ts = host.make_dpm_schedule(case["S"], ACP, case["discretize"])["ddim_timesteps"]
    alphas = plms_ref.alpha_generator(len(ts), case["alpha_type"])
    b = inp["x"].shape[0]

    def eps_fn(x, t, i):
        with torch.no_grad():
            return oracle_eps(T(x).float(), torch.full((b,), t, dtype=torch.long), i, alphas[i]).double().numpy()
    blend = None
    if case["mask"]:
        draw, rec = dc.recorder(name + ".noise")
        acp64 = np.cumprod(1.0 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2, axis=0)
        sac, s1ac = np.sqrt(acp64).astype(np.float32), np.sqrt(1.0 - acp64).astype(np.float32)       # q_sample's fp32 buffers (ldm.py:19-22)
        x0, mask = inp["x0"].double().numpy(), inp["mask"].double().numpy()

        def blend(x, t):
            img_orig = float(sac[t]) * x0 + float(s1ac[t]) * draw(inp["x0"]).double().numpy()
            return img_orig * mask + (1.0 - mask) * x
    return T(dr.dpmpp_sample(eps_fn, inp["x"].double().numpy(), ts, ACP, case["order"], blend=blend)), len(ts)


def run_dpm(model, case, inp, randn_like=None):
    model.first_conv_type = "GLIGEN"
    s = DPMSolverSampler(LatentDiffusion(device=DEV), model, order=case["order"], discretize=case["discretize"], **tgd._callbacks(case["alpha_type"]))
    with dc.patched_randn_like(randn_like if randn_like is not None else torch.randn_like):
        out = s.sample(S=case["S"], shape=tuple(inp["x"].shape), input=tgd._input(model, inp), uc=inp["uc"], guidance_scale=case["guidance"],
                       mask=inp.get("mask"), x0=inp.get("x0"))
    model.first_conv_type = "GLIGEN"
    return out


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dpm_sampler_matches_the_float64_loop(case, strict):
    inp = case_inputs(case["name"])
    ref, n = reference(case["name"])
    assert torch.isfinite(ref).all() and n <= case["S"]
    model = tgd.get_model(case["unet"], strict)
    rec_fn, rec = dc.recorder(case["name"] + ".noise")
    out = run_dpm(model, case, inp, rec_fn)
    # the RNG contract: no draw without a mask; with one, exactly one randn_like(x0) per step
    assert [tuple(a.shape) for a in rec] == ([tuple(inp["x0"].shape)] * n if case["mask"] else [])
    assert torch.isfinite(out).all() and tuple(out.shape) == tuple(inp["x"].shape)
    r_dpm, r_plms = tgd.rel_l2(out.double(), ref), tgd.plms_error(case["unet"], strict)
    print(f"[dpmpp_parity] {case['name']:24s} {'strict' if strict else 'default':8s} n = {n:2d}   r_dpmpp = {r_dpm:.3e}   r_plms = {r_plms:.3e}   "
          f"ratio = {r_dpm / r_plms:.2f}   (bound: ratio < 2)")
    assert r_dpm < 2 * r_plms, (r_dpm, r_plms)


# ------------------------------------------------------------------------------------------- 9. determinism
def test_no_mask_is_seed_independent_and_a_mask_draws_once_per_step():
    model = tgd.get_model("norel")
    case = CASES[0]
    inp = case_inputs(case["name"])
    torch.manual_seed(1)
    a = run_dpm(model, case, inp).clone()
    torch.manual_seed(2)
    b = run_dpm(model, case, inp).clone()
    assert torch.equal(a, b), "without a mask the result is bit-equal whatever the torch seed"
    o1 = run_dpm(model, dict(case, order=1), inp)
    assert tgd.rel_l2(o1, a) > 1e-3, "order 1 is another solver"
    # with a mask: exactly one randn_like(x0) per step, and the result follows those draws
    mcase = CASES[-1]
    minp = case_inputs(mcase["name"])
    rel = tgd.get_model("rel")
    n = len(host.make_dpm_schedule(mcase["S"], ACP, mcase["discretize"])["ddim_timesteps"])
    f1, r1 = dc.recorder("dpmpp.det.a")
    m1 = run_dpm(rel, mcase, minp, f1).clone()
    assert [tuple(t.shape) for t in r1] == [tuple(minp["x0"].shape)] * n
    m2 = run_dpm(rel, mcase, minp, dc.replayer(r1)[0]).clone()
    assert torch.equal(m1, m2), "the same draws give the same bits"
    m3 = run_dpm(rel, mcase, minp, dc.recorder("dpmpp.det.b")[0])
    assert not torch.equal(m3, m1), "other draws give another latent"


# ------------------------------------------------------------------------------------------- 10. the public switch
LOC = [[0.10, 0.10, 0.50, 0.55], [0.55, 0.20, 0.90, 0.70]]


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ckpt_dpmpp") / "tiny_gligen_text.pth")
    stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)      # 16 x 16 latents <-> 32 x 32 images
    stubs.install_fake_sng_parser()
    return p, itf.load_all_models(p, DEV), stubs.toy_clip().to(DEV), stubs.ToyProcessor()


_same = tgd._same


def _images_ok(ims, n):
    return len(ims) == n and all(im.size == (32, 32) and im.mode == "RGB" and np.asarray(im).std() > 0 for im in ims)


def test_public_switch(loaded):
    p, am, clip, proc = loaded
    model = am[0]
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5])
    noise = T(recipe.normal("gpudpmpp.noise", (2, 4, 16, 16), 9))
    base = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=8)

    def run(**more):
        model.first_conv_type = "GLIGEN"
        torch.manual_seed(len(more))                                          # the seed must not matter
        return itf.run_one_image(am, dict(base, **more), dict(meta), noise.clone().to(DEV), clip, proc, device=DEV)
    today = run()
    d = run(sampler="dpmpp_2m")
    assert _images_ok(d, 2) and not _same(d, today), "another sampler, other images than PLMS"
    assert _same(d, run(sampler="dpmpp_2m")), "the same call twice is bitwise equal"
    assert _same(d, run(sampler="dpmpp_2m", dpm_order=2, dpm_discretize="logsnr")), "the defaults, spelled out"
    assert not _same(d, run(sampler="dpmpp_2m", dpm_order=1)) and not _same(d, run(sampler="dpmpp_2m", dpm_discretize="uniform"))
    assert _same(today, run()), "the switch is per call: the next call without it runs PLMS"
    with pytest.raises(ValueError, match="dpm_order"):
        run(dpm_order=1)
    model.first_conv_type = "GLIGEN"
    bmeta = dict(prompts=[meta["prompt"]] * 2, phrases=[meta["phrases"]] * 2, locations=[LOC] * 2, alpha_type=meta["alpha_type"])
    bt = itf.run_batch_images(am, dict(base, sampler="dpmpp_2m"), dict(bmeta), noise.clone().to(DEV), clip, proc, device=DEV)
    assert _images_ok(bt, 2)
    model.first_conv_type = "GLIGEN"
    assert _same(bt, itf.run_batch_images(am, dict(base, sampler="dpmpp_2m"), dict(bmeta), noise.clone().to(DEV), clip, proc, device=DEV))
    gi._MODELS[p] = am
    try:
        cfg = dict(batch_size=1, guidance_scale=7.5, no_plms=False, device=DEV, steps=8)
        m1 = dict(ckpt=p, prompt=meta["prompt"], phrases=meta["phrases"], locations=LOC)

        def grun(**more):
            return gi.run(m1, dict(cfg, **more), starting_noise=noise[:1].clone().to(DEV), clip_model=clip, clip_processor=proc)
        a, b = grun(), grun(sampler="dpmpp_2m")
        assert _images_ok(b, 1) and not _same(a, b)
        assert _same(b, grun(sampler="dpmpp_2m")) and _same(a, grun(sampler="plms"))
    finally:
        gi._MODELS.pop(p, None)


def test_public_switch_txt2img(loaded):
    p, am, clip, proc = loaded
    policy = type("P", (), dict(device=DEV, select=lambda self, e, f, k: torch.zeros(1, k, dtype=torch.long)))()
    pool = type("Pool", (), dict(towers=object(), features=None, examples=[{"captions": "a cat on a mat", "label": ["cat"], "bbox": [[0.5, 0.5, 0.4, 0.4]]}]))()
    llm = lambda text: "cat: [0.10, 0.10, 0.40, 0.45]\nmat: [0.05, 0.60, 0.90, 0.35]"
    noise = T(recipe.normal("gpudpmpp.t2i.noise", (2, 4, 16, 16), 9))
    real = txt2img.embed_texts
    txt2img.embed_texts = lambda towers, tokenize, texts: torch.zeros(1, 8)       # the selection is not under test here
    try:
        def gen(**more):
            am[0].first_conv_type = "GLIGEN"
            return txt2img.generate(am, policy, pool, "cat sitting on mat", llm, None, clip, proc, shot_number=1, num_per_prompt=2, batch_size=2,
                                    steps=8, starting_noise=noise, device=DEV, **more)["images"]
        a, b = gen(), gen(sampler="dpmpp_2m")
        assert _images_ok(b, 2) and not _same(a, b)
        assert _same(b, gen(sampler="dpmpp_2m"))
    finally:
        txt2img.embed_texts = real
