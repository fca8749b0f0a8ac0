"""Image-to-image (SDEdit: sampling from a noised input image, ``strength``) on the GPU: gl_q_sample against the torch fp32 expression
(bitwise), ``sample_from`` of the three samplers against a loop written here from ``engine.forward``, the combine ops and the op-level
updates (bitwise, the draws replayed, the fuser schedule of the steps that run), its identity with ``sample()`` at strength 1, its
composition with the masked blend, rectangular latents and three-branch guidance, what the image and the strength change, and the public
entries on synthetic checkpoints.

The models and helpers are test_gpu_ddim's and test_gpu_cfg3's: one set of TINY engines serves the sampler test files."""
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
import test_gpu_cfg3 as tg3
import test_gpu_ddim as tgd
from layoutllm_t2i_amd import _lib, host, ops, recipe, txt2img
from layoutllm_t2i_amd import gligen_inference as gi
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.model import LatentDiffusion

DEV = "cuda:0"
T = torch.from_numpy
KEY = "strength"
rel_l2 = tgd.rel_l2


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


# ------------------------------------------------------------------------------------------- 1. the kernel
A, S1 = float(np.float32(0.6123724)), float(np.float32(0.7905694))
# (noise's shape, x0's batch): [1, 4, 8, 8] (256) and [2, 4, 8, 16] (1024: more than one block of float4s) take the float4 path, the latter
# with one image for both samples and with one each; [1, 3, 5, 7] (105) the scalar one
KSHAPES = [((1, 4, 8, 8), 1), ((2, 4, 8, 16), 1), ((2, 4, 8, 16), 2), ((1, 3, 5, 7), 1)]


def _operands(shape, nb0):
    tag = "i2i.k." + "x".join(map(str, shape)) + f".{nb0}"
    x0 = T(recipe.normal(tag + ".x0", (nb0,) + tuple(shape[1:]), 3)).to(DEV)
    noise = T(recipe.normal(tag + ".noise", shape, 3)).to(DEV)
    return x0, noise


@pytest.mark.parametrize("shape,nb0", KSHAPES, ids=["x".join(map(str, s)) + f"-x0b{b}" for s, b in KSHAPES])
def test_q_sample_is_bitwise_the_torch_expression(shape, nb0):
    x0, noise = _operands(shape, nb0)
    keep0, keepn = x0.clone(), noise.clone()
    ref = A * x0 + S1 * noise
    assert tuple(ref.shape) == shape and torch.isfinite(ref).all()
    out = torch.full(shape, float("nan"), device=DEV)
    got = ops.q_sample(x0, noise, A, S1, out=out)
    assert got is out and torch.equal(out, ref), float((out - ref).abs().max())
    assert torch.equal(x0, keep0) and torch.equal(noise, keepn), "the inputs are unchanged"
    new = ops.q_sample(x0, noise, A, S1)
    assert new.data_ptr() not in (x0.data_ptr(), noise.data_ptr()) and torch.equal(new, ref)
    # in place on the noise, as the sampler's running latent would take it
    got = ops.q_sample(x0, noise, A, S1, out=noise)
    assert got is noise and torch.equal(noise, ref) and torch.equal(x0, keep0)


def test_q_sample_on_unaligned_pointers():
    """256 elements starting 4 bytes behind a 16-byte boundary: an aligned n on the scalar path; nothing is written outside the view"""
    base = {k: T(recipe.normal(f"i2i.k.un.{k}", (2 * 256 + 8,), 3)).to(DEV) for k in ("x0", "noise", "out")}
    for nb0 in (1, 2):
        x0 = base["x0"][1:1 + nb0 * 256].view(nb0, 4, 8, 8)
        noise = base["noise"][1:513].view(2, 4, 8, 8)
        whole = base["out"].clone()
        out = whole[1:513].view(2, 4, 8, 8)
        assert x0.data_ptr() % 16 == 4 and noise.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
        ref = A * x0 + S1 * noise
        ops.q_sample(x0, noise, A, S1, out=out)
        assert torch.equal(out, ref)
        assert torch.equal(whole[:1], base["out"][:1]) and torch.equal(whole[513:], base["out"][513:]), "nothing written around the view"


def test_q_sample_refuses_bad_operands():
    x0, noise = torch.zeros(1, 4, 8, 8, device=DEV), torch.zeros(2, 4, 8, 8, device=DEV)
    for bad0, badn, bado in ((torch.zeros(3, 4, 8, 8, device=DEV), noise, None), (torch.zeros(1, 4, 8, 16, device=DEV), noise, None),
                             (torch.zeros(1, 3, 8, 8, device=DEV), noise, None), (x0, noise, torch.zeros(1, 4, 8, 8, device=DEV)),
                             (x0, noise.view(-1), None), (x0, noise[:, :, ::2], None), (x0[:, :, ::2], noise[:, :, ::2].contiguous(), None)):
        with pytest.raises(ValueError):
            ops.q_sample(bad0, badn, A, S1, out=bado)
    with pytest.raises(TypeError):
        ops.q_sample(x0.double(), noise, A, S1)
    with pytest.raises(_lib.HipLibraryError):
        ops.q_sample(x0.cpu(), noise, A, S1)
    with pytest.raises(_lib.HipLibraryError):
        ops.q_sample(x0, noise.cpu(), A, S1)
    lib = _lib.lib()
    p, q = x0.data_ptr(), noise.data_ptr()
    assert lib.gl_q_sample(p, q, A, S1, 2, 256, 3, q, None) == -1
    assert lib.gl_q_sample(p, q, A, S1, 0, 256, 1, q, None) == -1
    assert lib.gl_q_sample(p, q, A, S1, 2, 0, 1, q, None) == -1
    assert lib.gl_q_sample(None, q, A, S1, 2, 256, 1, q, None) == -1


# ------------------------------------------------------------------------------------------- 2. the samplers against a loop written here
S, G, ETA, STRENGTH = tg3.S, tg3.G, tg3.ETA, 0.5
ALPHA, CLASSES, ACP = tg3.ALPHA, tg3.CLASSES, tg3.ACP
THREE, TWO = tg3.THREE, tg3.TWO


def _inputs(cfg, b, hw, seed):
    return tg3._inputs(cfg, b, hw, seed)


def _z0(shape, tag="i2i.z0"):
    """an 'encoded image': recipe noise at the latent's scale"""
    return T((recipe.normal(tag, shape, 5) * np.float32(0.8)).astype(np.float32))


def _coefs(t):
    ld = LatentDiffusion(device=DEV)
    return float(ld.sqrt_alphas_cumprod.cpu().numpy()[int(t)]), float(ld.sqrt_one_minus_alphas_cumprod.cpu().numpy()[int(t)])


def run_from(model, name, inp, alpha_type, z0, strength, randn_like, layout=None, steps=S):
    """``sample_from`` on the case; returns (latent, how often set_alpha_scale was called)"""
    cls, kw = CLASSES[name]
    model.first_conv_type = "GLIGEN"
    cb = tgd._callbacks(alpha_type)
    calls = []
    real = cb["set_alpha_scale"]
    cb["set_alpha_scale"] = lambda m, a: calls.append(a) or real(m, a)
    s = cls(LatentDiffusion(device=DEV), model, **kw, **cb)
    with dc.patched_randn_like(randn_like):
        out = s.sample_from(steps, tuple(inp["x"].shape), tgd._input(model, inp), inp["uc"], G, z0, strength, mask=inp.get("mask"),
                            x0=inp.get("x0"), layout_guidance_scale=layout).clone()
    model.first_conv_type = "GLIGEN"
    return out, calls


def manual_loop(model, name, inp, alpha_type, z0, strength, randn_like, layout=None):
    """the truncated sampler restated: the noised start as the torch expression, then per step the blend, one evaluation (2B + cfg_combine;
    under a layout scale 3B + cfg3_combine where the step can see the grounding) and the sampler's op-level update on the B-sized guided eps.
    Returns (latent, the batch form of every evaluation, the number of steps)."""
    eng = model.engine
    sched = {"plms": lambda: host.make_schedule(S, ACP), "ddim": lambda: host.make_ddim_schedule(S, ACP, "uniform", ETA),
             "dpmpp_2m": lambda: host.make_dpm_schedule(S, ACP, "logsnr")}[name]()
    full = [int(t) for t in np.flip(sched["ddim_timesteps"])]
    n_run = host.img2img_run_steps(len(full), strength)
    ts = full[len(full) - n_run:]
    alphas = host.alpha_generator(n_run, alpha_type)
    ld = LatentDiffusion(device=DEV)
    sac, s1ac = ld.sqrt_alphas_cumprod.cpu().numpy(), ld.sqrt_one_minus_alphas_cumprod.cpu().numpy()
    noise0 = inp["x"].to(DEV, torch.float32).contiguous()
    x = (float(sac[ts[0]]) * z0.to(DEV) + float(s1ac[ts[0]]) * noise0).contiguous()          # q_sample(z0, t0), ldm.py:19-22
    assert x.shape == noise0.shape
    state = dict(form=None, sd=False, forms=[])

    def guided(x_eval, t, alpha):
        want = THREE if layout is not None and c3.needs_text_branch(model.cfg.relation, alpha) else TWO
        if want != state["form"]:
            tg3._set(model, inp, want)
            state["form"] = want
        state["forms"].append(len(want))
        eps = eng.forward(x_eval, float(t), alpha, state["sd"], len(want))
        e = torch.empty_like(x_eval)
        return ops.cfg3_combine(eps, G, layout, e) if want is THREE else ops.cfg_combine(eps, G, e)

    old, prev = [], None
    hist = torch.empty_like(x)
    with dc.patched_randn_like(randn_like):
        for i, t in enumerate(ts):
            index, alpha = n_run - i - 1, alphas[i]
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
                    e_next = guided(x_mid, ts[min(i + 1, n_run - 1)], alpha)
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
                sq_at, s1m, c_x, c_d, w1, w0 = host.dpm_step_coefs(sched, index, prev, 2, n_nodes=n_run)
                e = guided(x, t, alpha)
                ops.dpmpp_update(e, x, x, hist, sqrt_at=sq_at, s1m=s1m, c_x=c_x, c_d=c_d, w1=w1, w0=w0, x0_old=hist if w0 != 0 else None)
                prev = index
    return x, state["forms"], n_run


def _check_sampler(unet, name, inp, layout=None):
    model = tgd.get_model(unet)
    z0 = _z0((1,) + tuple(inp["x"].shape[1:]))
    rec_fn, rec = dc.recorder(f"i2i.{unet}.{name}.noise")
    out, calls = run_from(model, name, inp, ALPHA[unet], z0, STRENGTH, rec_fn, layout)
    replay, st = dc.replayer(rec)
    want, forms, n_run = manual_loop(model, name, inp, ALPHA[unet], z0, STRENGTH, replay, layout)
    assert st["n"] == len(rec), "the sampler drew exactly what the loop draws, in its order"
    assert torch.isfinite(want).all() and torch.equal(out, want), float((out - want).abs().max())
    assert 1 < n_run < S and len(calls) == n_run and calls == host.alpha_generator(n_run, ALPHA[unet]), "the fuser schedule of the steps that run"
    print(f"[img2img_parity] {unet:5s} {name:8s} {tuple(inp['x'].shape)} strength {STRENGTH}{' masked' if 'mask' in inp else ''}"
          f"{' layout scale ' + str(layout) if layout is not None else ''}: {n_run} nodes, {len(forms)} evaluations, {len(rec)} draws, "
          f"max |sample_from - restated loop| = {float((out - want).abs().max()):.1e} (bitwise)")
    return out, forms


@pytest.mark.parametrize("name", list(CLASSES))
@pytest.mark.parametrize("unet", ["rel", "norel"])
def test_sample_from_equals_the_restated_loop(unet, name):
    model = tgd.get_model(unet)
    _check_sampler(unet, name, _inputs(model.cfg, 1, (8, 8), seed=51))


# ------------------------------------------------------------------------------------------- 3. strength 1 is sample() from the noised image
@pytest.mark.parametrize("name", list(CLASSES))
def test_strength_one_is_sample_from_the_noised_image(name):
    model = tgd.get_model("norel")
    inp = _inputs(model.cfg, 1, (8, 8), seed=52)
    z0 = _z0((1, 4, 8, 8))
    draw = lambda: dc.recorder(f"i2i.one.{name}.noise")[0]
    out, calls = run_from(model, name, inp, ALPHA["norel"], z0, 1.0, draw())
    cls, kw = CLASSES[name]
    model.first_conv_type = "GLIGEN"
    s = cls(LatentDiffusion(device=DEV), model, **kw, **tgd._callbacks(ALPHA["norel"]))
    s.make_schedule(S, *s._sample_schedule)
    t_top = int(np.flip(s.ddim_timesteps)[0])
    assert len(calls) == len(s.ddim_timesteps)
    start = ops.q_sample(z0.to(DEV), inp["x"].to(DEV).contiguous(), *_coefs(t_top))
    with dc.patched_randn_like(draw()):
        want = s.sample(S=S, shape=tuple(inp["x"].shape), input=tgd._input(model, dict(inp, x=start)), uc=inp["uc"], guidance_scale=G).clone()
    model.first_conv_type = "GLIGEN"
    assert torch.isfinite(want).all() and torch.equal(out, want), float((out - want).abs().max())
    # ... which is not sample() from the noise alone: the image reaches the result even at strength 1
    with dc.patched_randn_like(draw()):
        plain = s.sample(S=S, shape=tuple(inp["x"].shape), input=tgd._input(model, inp), uc=inp["uc"], guidance_scale=G).clone()
    model.first_conv_type = "GLIGEN"
    assert rel_l2(out, plain) > 1e-3


# ------------------------------------------------------------------------------------------- 4. composition
def test_masked_rectangular_dpm_equals_the_restated_loop():
    for unet in ("rel", "norel"):
        model = tgd.get_model(unet)
        inp = _inputs(model.cfg, 1, (8, 16), seed=53)
        inp.update({k: T(v) for k, v in dc.mask_inputs(8, 16).items()})
        _check_sampler(unet, "dpmpp_2m", inp)


def test_layout_scale_plms_equals_the_restated_loop():
    model = tgd.get_model("norel")
    out, forms = _check_sampler("norel", "plms", _inputs(model.cfg, 1, (8, 8), seed=54), layout=12.0)
    k = forms.index(2)
    assert 0 < k < len(forms) and set(forms[:k]) == {3} and set(forms[k:]) == {2}, "one conditioning switch per image"


# ------------------------------------------------------------------------------------------- 5. what the image and the strength change
def test_image_and_strength_matter_and_one_image_serves_the_batch():
    model = tgd.get_model("norel")
    inp = _inputs(model.cfg, 2, (8, 8), seed=55)
    draw = lambda: dc.recorder("i2i.effect.noise")[0]
    run = lambda z0, strength: run_from(model, "plms", inp, ALPHA["norel"], z0, strength, draw())[0]
    za, zb = _z0((1, 4, 8, 8), "i2i.za"), _z0((1, 4, 8, 8), "i2i.zb")
    a, b = run(za, 0.5), run(zb, 0.5)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    r_img, r_str = rel_l2(a, b), rel_l2(a, run(za, 1.0))
    print(f"[img2img_effect] rel_l2 between two init latents at strength 0.5 = {r_img:.3e}; between strengths 0.5 and 1.0 = {r_str:.3e}")
    assert r_img > 1e-3 and r_str > 1e-3
    assert torch.equal(a, run(za, 0.5)), "the same call twice"
    assert torch.equal(a, run(za.repeat(2, 1, 1, 1), 0.5)), "[1, ...] is the explicit repeat, bitwise"
    assert rel_l2(run(torch.cat([za, zb], 0), 0.5)[1:], a[1:]) > 1e-3, "with one image per sample, sample 1 sees its own"
    for bad in (torch.zeros(3, 4, 8, 8), torch.zeros(1, 4, 8, 16), torch.zeros(2, 4, 8, 8).double()):
        launches = model.engine.num_launches()
        with pytest.raises(ValueError, match="init_latent"):
            run(bad, 0.5)
        assert model.engine.num_launches() == launches


# ------------------------------------------------------------------------------------------- 6. the public entries
LOC = tg3.LOC
_same, _images_ok = tgd._same, tg3._images_ok


def _add_encoder(ck, path):
    """the VAE encoder's tensors into a synthetic checkpoint (stubs writes the decoder alone)"""
    ck["autoencoder"].update({k: T(np.asarray(v)) for k, v in recipe.vae_encoder_state_dict(VAE_TINY, 0).items()})
    torch.save(ck, path)


@pytest.fixture(scope="module")
def text_ckpt(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ckpt_i2i") / "tiny_gligen_text.pth")
    ck = stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)      # 16 x 16 latents <-> 32 x 32 images
    _add_encoder(ck, p)
    stubs.install_fake_sng_parser()
    return p, itf.load_all_models(p, DEV), stubs.toy_clip().to(DEV), stubs.ToyProcessor()


def _picture(seed, size=(48, 40)):
    """a PIL image of another size than the model's: smooth colour gradients plus a little noise"""
    from PIL import Image
    w, h = size
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx / w, yy / h, (xx + yy) / (w + h)], -1) * rng.uniform(0.3, 1.0, 3)
    return Image.fromarray(np.clip((base + rng.normal(0, 0.05, base.shape)) * 255, 0, 255).astype(np.uint8))


META = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5])
BASE = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)          # 4 steps: 2 nodes run at strength 0.5
NOISE = T(recipe.normal("gpui2i.noise", (2, 4, 16, 16), 9))


def _run_text(am, clip, proc, image=None, meta=None, **more):
    am[0].first_conv_type = "GLIGEN"
    torch.manual_seed(7)
    m = dict(META if meta is None else meta)
    if image is not None:
        m["init_image"] = image
    return itf.run_one_image(am, dict(BASE, **more), m, NOISE.clone().to(DEV), clip, proc, device=DEV)


def test_run_one_image_takes_an_init_image_and_keeps_no_state(text_ckpt):
    p, am, clip, proc = text_ckpt
    pic = _picture(1)
    plain = _run_text(am, clip, proc)
    keyed = _run_text(am, clip, proc, pic, **{KEY: 0.5})
    assert _images_ok(keyed, 2) and _same(keyed, _run_text(am, clip, proc, pic, **{KEY: 0.5})) and not _same(keyed, plain)
    assert not _same(keyed, _run_text(am, clip, proc, _picture(2), **{KEY: 0.5})), "another picture, other images"
    assert not _same(keyed, _run_text(am, clip, proc, pic, **{KEY: 1.0})), "another strength, other images"
    default = _run_text(am, clip, proc, pic)                           # the cached config holds strength = 1.0 by now: the call decides
    assert _same(default, _run_text(am, clip, proc, pic, **{KEY: 0.75})) and not _same(default, _run_text(am, clip, proc, pic, **{KEY: 1.0}))
    after = _run_text(am, clip, proc)
    fresh = _run_text(itf.load_all_models(p, DEV), clip, proc)         # a handle that has never seen the keys
    assert _same(after, fresh) and _same(after, plain), "the feature leaves no state behind"


def test_every_sampler_batch_entry_and_the_other_entries_take_the_keys(text_ckpt, tmp_path):
    p, am, clip, proc = text_ckpt
    pic = _picture(1)
    path = str(tmp_path / "init.png")
    pic.save(path)
    keyed = _run_text(am, clip, proc, pic, **{KEY: 0.5})
    assert _same(keyed, _run_text(am, clip, proc, path, **{KEY: 0.5})), "a path is the image"
    assert _images_ok(_run_text(am, clip, proc, pic, sampler="dpmpp_2m", **{KEY: 0.5}), 2)
    assert _images_ok(_run_text(am, clip, proc, pic, sampler="ddim", ddim_eta=0.5, **{KEY: 0.5}), 2)
    assert _images_ok(_run_text(am, clip, proc, pic, layout_guidance_scale=12, **{KEY: 0.5}), 2)
    # inpainting and image-to-image together, on a rectangular latent
    am[0].first_conv_type = "GLIGEN"
    torch.manual_seed(7)
    rect = T(recipe.normal("gpui2i.rect", (2, 4, 16, 24), 9)).to(DEV)
    both = itf.run_one_image(am, dict(BASE, **{KEY: 0.5}), dict(META, init_image=pic, input_image=_picture(3)), rect, clip, proc, device=DEV)
    assert len(both) == 2 and all(im.size == (48, 32) and np.asarray(im).std() > 0 for im in both)
    # run_batch_images: a list with one image per sample, or one for all
    bmeta = dict(prompts=[META["prompt"]] * 2, phrases=[META["phrases"]] * 2, locations=[LOC] * 2, alpha_type=META["alpha_type"])

    def batch(images):
        am[0].first_conv_type = "GLIGEN"
        torch.manual_seed(7)
        return itf.run_batch_images(am, dict(BASE, **{KEY: 0.5}), dict(bmeta, init_image=images), NOISE.clone().to(DEV), clip, proc, device=DEV)
    two = batch([pic, _picture(2)])
    # (one picture for all is encoded once, with one sample's posterior noise: not the bits of the list of two copies)
    assert _images_ok(two, 2) and _same(two, batch([pic, _picture(2)])) and not _same(two, batch([pic, pic])) and _images_ok(batch(pic), 2)
    # gligen_inference.run: both keys in its config
    gi._MODELS[p] = am
    try:
        cfg = dict(batch_size=1, guidance_scale=7.5, no_plms=False, device=DEV, steps=4)
        m1 = dict(ckpt=p, prompt=META["prompt"], phrases=META["phrases"], locations=LOC)

        def grun(**more):
            torch.manual_seed(7)
            return gi.run(m1, dict(cfg, **more), starting_noise=NOISE[:1].clone().to(DEV), clip_model=clip, clip_processor=proc)
        a, b = grun(), grun(init_image=pic, strength=0.5)
        assert _images_ok(b, 1) and not _same(a, b) and _same(b, grun(init_image=pic, strength=0.5)) and _same(a, grun())
        with pytest.raises(ValueError, match=KEY):
            grun(strength=0.5)
    finally:
        gi._MODELS.pop(p, None)
    # txt2img.generate: init_image= / strength=
    policy = type("P", (), dict(device=DEV, select=lambda self, e, f, k: torch.zeros(1, k, dtype=torch.long)))()
    pool = type("Pool", (), dict(towers=object(), features=None, examples=[{"captions": "a cat on a mat", "label": ["cat"], "bbox": [[0.5, 0.5, 0.4, 0.4]]}]))()
    llm = lambda text: "cat: [0.10, 0.10, 0.40, 0.45]\nmat: [0.05, 0.60, 0.90, 0.35]"
    real = txt2img.embed_texts
    txt2img.embed_texts = lambda towers, tokenize, texts: torch.zeros(1, 8)       # the selection is not under test here
    try:
        def gen(**more):
            am[0].first_conv_type = "GLIGEN"
            torch.manual_seed(7)
            return txt2img.generate(am, policy, pool, "cat sitting on mat", llm, None, clip, proc, shot_number=1, num_per_prompt=2, batch_size=2,
                                    steps=4, starting_noise=NOISE, device=DEV, **more)["images"]
        a, b = gen(), gen(init_image=pic, strength=0.5)
        assert _images_ok(b, 2) and not _same(a, b) and _same(b, gen(init_image=pic, strength=0.5))
    finally:
        txt2img.embed_texts = real


def test_refusals_come_before_any_encoder_or_kernel(text_ckpt):
    p, am, clip, proc = text_ckpt
    pic = _picture(1)
    eng = am[0].engine
    _run_text(am, clip, proc)
    launches, cond = eng.num_launches(), eng.cond
    for image, more, names in ((pic, {KEY: 0}, KEY), (pic, {KEY: True}, KEY), (None, {KEY: 0.5}, KEY)):
        with pytest.raises(ValueError, match=names):
            _run_text(am, clip, proc, image, **more)
    bmeta = dict(prompts=[META["prompt"]] * 2, phrases=[META["phrases"]] * 2, locations=[LOC] * 2, alpha_type=META["alpha_type"])
    with pytest.raises(ValueError, match="init_image"):
        itf.run_batch_images(am, dict(BASE, **{KEY: 0.5}), dict(bmeta, init_image=[pic] * 3), NOISE.clone().to(DEV), clip, proc, device=DEV)
    assert eng.num_launches() == launches and eng.cond is cond


def test_keypoint_checkpoint_takes_an_init_image(tmp_path):
    import test_gpu_kp as tkp
    p = str(tmp_path / "tiny_gligen_keypoint.pth")
    tkp._write_kp_checkpoint(p, 3)
    _add_encoder(torch.load(p, weights_only=False), p)
    am = itf.load_all_models(p, DEV)
    locations = np.load(os.path.join(tgd.GOLD, "kp_prepare_batch.npz"))["locations"].tolist()
    meta = dict(prompt="A young man and a small boy are talking", locations=locations, alpha_type=[0.5, 0.0, 0.5])
    plain = _run_text(am, None, None, meta=meta)
    keyed = _run_text(am, None, None, _picture(1), meta=meta, **{KEY: 0.5})
    assert _images_ok(keyed, 2) and not _same(plain, keyed) and _same(keyed, _run_text(am, None, None, _picture(1), meta=meta, **{KEY: 0.5}))
    assert _same(plain, _run_text(am, None, None, meta=meta))
