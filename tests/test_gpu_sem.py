"""The semantic-map grounding family (GLIGEN's checkpoint_generation_sem.pth) on the GPU: the three kernels of csrc/sem.hip against their
torch expressions, both input forms (class map and float one-hot), the tokenizer against tests/sem_ref.py and the reference's own outputs, the
downsampler and TINY-width UNets against ``openaimodel_original`` goldens (tests/golden/sem_*.npz), batched CFG, and the interface on a
synthetic sem checkpoint.  Bad arguments are checked by return code on the host (tests/test_sem_host.py): nothing here provokes a fault."""
import dataclasses
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import sem_cases as sm
import sem_ref
import sp_ref
import stubs
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import ops, recipe, semantic
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.model import SemGroundingNetInput, UNetModel
from test_gpu_model import rel_l2, report

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
NAN = float("nan")
KEYS = sem_ref.KEYS


def rnd(tag, shape, scale=1.0):
    return T(recipe.normal(f"gpusem.{tag}", tuple(shape), 47)) * scale


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


# ------------------------------------------------------------------------------------------- the gather conv
FORMS = {"in_conv": (3, 1, 1, 3, False), "ds": (4, 2, 1, 16, True)}          # (K, stride, pad, Co, SiLU): the tokenizer's and the downsampler's
SHAPES = [(24, 24, 16), (16, 16, 16), (8, 12, 16)]                           # (Hs, Ws, R): non-integer ratio, identity, upsample and non-square


def _gather(cm, R, w, b, K, s, p, silu, sentinel=True):
    B, Co = cm.shape[0], w.shape[0]
    Ro = (R + 2 * p - K) // s + 1
    n, G = B * Co * Ro * Ro, 64
    buf = torch.full((2 * G + n,), NAN, device=DEV)
    out = ops.sem_gather_conv(cm.to(DEV), R, semantic.gather_table(w).to(DEV), b.to(DEV), K, s, p, silu, buf[G:G + n].view(B, Co, Ro, Ro))
    h = buf.cpu()
    assert torch.isnan(h[:G]).all() and torch.isnan(h[G + n:]).all(), "sentinel overwritten"
    return out.cpu()


@pytest.mark.parametrize("C", [152, 5])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("Hs,Ws,R", SHAPES, ids=[f"{h}x{w}-R{r}" for h, w, r in SHAPES])
def test_gather_conv(Hs, Ws, R, form, C):
    """F.conv2d(F.interpolate(onehot, R), W, b) (+ SiLU) in torch fp32 on the CPU, rtol 1e-5 / atol 1e-6 (the tolerance of
    test_gpu_sp.py::test_conv4x4s2): both sides sum at most K^2 + 1 non-zero fp32 terms.  B = 2 with different maps; the output buffer starts
    as NaN with NaN sentinels around it."""
    K, s, p, Co, silu = FORMS[form]
    B = 2
    cm = T(sm.class_map(f"gc{Hs}.{Ws}", B, Hs, Ws, C, seed=47))
    assert not torch.equal(cm[0], cm[1]) and int(cm.max()) == C - 1 and int(cm.min()) == 0
    w, b = rnd(f"gcw{form}{C}", (Co, C, K, K)) * 0.3, rnd(f"gcb{form}", (Co,)) * 0.1
    out = _gather(cm, R, w, b, K, s, p, silu)
    ref = F.conv2d(F.interpolate(sem_ref.onehot(cm, C), (R, R)), w, b, stride=s, padding=p)
    ref = F.silu(ref) if silu else ref
    assert out.shape == ref.shape and torch.isfinite(out).all()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("form", list(FORMS))
def test_gather_conv_of_a_constant_map(form):
    """one class everywhere: away from the border every output of a channel is ONE constant, bias + the sum of that class's K^2 taps; on the
    border the out-of-image taps contribute nothing (zero padding of a one-hot is no class), so rows / columns there hold smaller sums"""
    K, s, p, Co, _ = FORMS[form]
    C, cls, R = 152, 151, 16
    cm = torch.full((1, 16, 16), cls, dtype=torch.uint8)
    w, b = rnd(f"ccw{form}", (Co, C, K, K)).abs() * 0.3 + 0.01, rnd(f"ccb{form}", (Co,)) * 0.1        # positive taps: fewer taps, smaller sums
    out = _gather(cm, R, w, b, K, s, p, False)[0]
    inner = out[:, 1:-1, 1:-1]
    assert torch.equal(inner, inner[:, :1, :1].expand_as(inner)), "one constant per channel away from the border"
    np.testing.assert_allclose(inner[:, 0, 0].numpy(), (b.double() + w[:, cls].double().sum((1, 2))).float().numpy(), rtol=1e-5, atol=1e-6)
    assert (out[:, 0, :] < inner[:, :1, 0]).all() and (out[:, :, 0] < inner[:, :1, 0]).all() and (out[:, 0, 0] < out[:, 0, 1]).all()
    np.testing.assert_allclose(out[:, 0, 0].numpy(), (b.double() + w[:, cls, p:, p:].double().sum((1, 2))).float().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("Co,n", [(8, 8), (8, 16), (1, 8), (1, 16)])
def test_sem_conv4x4s2(Co, n):
    """Conv2d(16, Co, 4, 2, 1) against F.conv2d, fp32: rtol 1e-5 / atol 1e-6 (256 fp32 products of O(1) values in a sum of O(1):
    sqrt(256) * 2^-24 = 1e-6 relative)"""
    B, Ci = 2, 16
    x, w, b = rnd(f"cvx{n}", (B, Ci, n, n)), rnd(f"cvw{Co}", (Co, Ci, 4, 4)) * (3.0 / (16 * Ci)) ** 0.5, rnd(f"cvb{Co}", (Co,)) * 0.1
    out = ops.sem_conv4x4s2(x.to(DEV), w.to(DEV), b.to(DEV), torch.full((B, Co, n // 2, n // 2), NAN, device=DEV))
    np.testing.assert_allclose(out.cpu().numpy(), F.conv2d(x, w, b, stride=2, padding=1).numpy(), rtol=1e-5, atol=1e-6)


def test_onehot_index():
    """[2, 152, 16, 24]: equal to argmax with count 0; a 0.5, a second 1.0 and an all-zero pixel planted in sample 1: counts [0, 3]"""
    B, C, H, W = 2, 152, 16, 24
    cm = T(sm.class_map("oh", B, H, W, C, seed=47))
    x = sem_ref.onehot(cm, C)
    out, bad = torch.full((B, H, W), 255, dtype=torch.uint8, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ops.sem_onehot_index(x.to(DEV), out, bad)
    assert torch.equal(out.cpu(), x.argmax(1).to(torch.uint8)) and torch.equal(out.cpu(), cm) and bad.cpu().tolist() == [0, 0]
    y = x.clone()
    y[1, int(cm[1, 3, 5]), 3, 5] = 0.5                         # not 1.0
    y[1, (int(cm[1, 7, 0]) + 1) % C, 7, 0] = 1.0               # a second 1.0
    y[1, :, 15, 23] = 0.0                                      # no class at all
    ops.sem_onehot_index(y.to(DEV), out, bad)
    assert bad.cpu().tolist() == [0, 3]
    assert torch.equal(out.cpu()[0], cm[0])


# ------------------------------------------------------------------------------------------- both input forms, the two stages
def _stages(case):
    cfg = sm.cfg_of(case)
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0).items() if k.startswith(("position_net.", "downsample_net."))}
    cmi = semantic.ClassMapInput(cfg.sem_classes, DEV)
    return cfg, sd, semantic.SemTokenizer(sd, cfg, DEV, cmi), semantic.SemDownsampler(sd, cfg, DEV, cmi), cmi


def test_both_input_forms():
    """the class map and its float one-hot give bit-identical tokens and downsampler output; one tensor object given to both stages is
    converted once; a sample that is not one-hot raises naming it, unless its mask is 0; a class id the model does not have raises"""
    case = sm.by_name("sem_unet_s1")
    cfg, sd, tok, ds, cmi = _stages(case)
    cm = T(sm.case_inputs(case)["sem"])
    oh, ones = sem_ref.onehot(cm, cfg.sem_classes), torch.ones(2)
    t_map, d_map = tok.tokens(cm, ones), ds(cm)
    calls = []
    real = ops.sem_onehot_index
    ops.sem_onehot_index = lambda *a: (calls.append(1), real(*a))[1]
    try:
        t_oh, d_oh = tok.tokens(oh, ones), ds(oh)
    finally:
        ops.sem_onehot_index = real
    assert len(calls) == 2, "one conversion per sample for the two stages"
    assert torch.equal(t_oh, t_map) and torch.equal(d_oh, d_map)
    assert tuple(t_map.shape) == (2, 4, 768) and tuple(d_map.shape) == (2, 8, 16, 16)
    dense = oh.clone()
    dense[1, :, 4, 4] = 1.0 / cfg.sem_classes
    with pytest.raises(ValueError, match="sample 1 is not one-hot: 1 of its pixels"):
        tok.tokens(dense, ones)
    with pytest.raises(ValueError, match="sample 1 is not one-hot"):
        ds(dense.clone())
    masked = tok.tokens(dense, torch.tensor([1.0, 0.0]))       # mask 0: neither converted nor validated
    assert torch.equal(masked[0], t_map[0]) and torch.equal(masked[1], tok.null_tokens()[0])
    zeros = tok.tokens(torch.zeros_like(oh), torch.zeros(2))   # the reference's null input
    assert torch.equal(zeros[0], tok.null_tokens()[0]) and torch.equal(zeros[1], tok.null_tokens()[0])
    with pytest.raises(ValueError, match="holds the value 152"):
        tok.tokens(torch.full((2, 8, 8), 152, dtype=torch.int64), ones)
    with pytest.raises(ValueError, match=r"need \[B, 152, H, W\]"):
        tok.tokens(torch.zeros(2, 5, 8, 8), ones)
    with pytest.raises(ValueError, match="mask has 3"):
        tok.tokens(cm, torch.ones(3))


@pytest.mark.parametrize("case", sm.POSNET_CASES, ids=[c["name"] for c in sm.POSNET_CASES])
def test_tokenizer_matches_sem_ref_and_the_reference(case):
    """T = 4 (resize 64 from 96 x 96), B = 2, sample 1 masked out, 152 and 5 classes: the method of
    test_gpu_sp.py::test_tokenizer_matches_sp_ref_and_the_reference.  The bound is MEASURED, fp16-operand sem_ref against fp32 sem_ref; the GPU
    result is within 2 x that of fp32 sem_ref and of the reference's own output; the masked-out sample is the cached null tokens bit for bit."""
    cfg, sd, tok, _, _ = _stages(case)
    inp = {a: T(v) for a, v in sm.case_inputs(case).items()}
    with torch.no_grad():
        ref32 = sem_ref.position_net(sd, cfg, inp["sem"], inp["mask"])
        ref16 = sem_ref.position_net(sd, cfg, inp["sem"], inp["mask"], q=sp_ref.fp16_operands)
    gold = T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"])
    out = tok.tokens(inp["sem"], inp["mask"])
    assert tuple(out.shape) == tuple(gold.shape) == (2, cfg.n_ground, cfg.pos_out_dim) and out.dtype == torch.float32
    bound = rel_l2(ref16, ref32)
    r, rg, re = rel_l2(out, ref32), rel_l2(out, gold), rel_l2(out, ref16)
    print(f"[{case['name']}] fp16-operand sem_ref vs fp32 sem_ref rel_l2 = {bound:.3e}; GPU vs fp32 sem_ref {r:.3e}, vs golden {rg:.3e}, "
          f"vs fp16-operand sem_ref {re:.3e}")
    assert torch.isfinite(out).all() and 1e-5 < bound < 1e-2
    assert r < 2 * bound and rg < 2 * bound, (r, rg, bound)
    null = tok.null_tokens()
    assert torch.equal(out[1], null[0]), "masked-out sample == cached null tokens"
    assert tok.null_tokens() is null
    assert rel_l2(out[0], null[0]) > 1e-2
    # the in_conv alone is fp32 on both sides: the gather against the conv of the one-hot
    np.testing.assert_allclose(tok.in_conv(inp["sem"].to(DEV)).cpu().numpy(), sem_ref.in_conv(sd, cfg, inp["sem"]).numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", sm.DS_CASES, ids=[c["name"] for c in sm.DS_CASES])
def test_downsampler_matches_reference_golden(case):
    """SemDownsampler (96 -> 64 -> 32 -> 16) against the reference's own output at rtol 1e-5 / atol 1e-6"""
    cfg, sd, _, ds, _ = _stages(case)
    out = ds(T(sm.case_inputs(case)["sem"]))
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    assert tuple(out.shape) == ref.shape == (case["B"], cfg.ds_out, cfg.ds_latent, cfg.ds_latent) and ds.out_side == 16
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------- whole model: tiny UNets vs the reference
_models = {}


def get_model():
    if "m" not in _models:
        cfg = sm.SEM_TINY
        m = UNetModel(cfg, recipe.state_dict(cfg, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(cfg, 0))
        m.grounding_tokenizer_input = SemGroundingNetInput()
        _models["m"] = m
    return _models["m"]


def _load(case):
    return {a: T(v) for a, v in sm.case_inputs(case).items()}, T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"])


def _golden_call(model, case, inp, extra=None):
    model.fuser_scale = case["scale"]
    model.first_conv_type = "SD" if case["sdconv"] else "GLIGEN"
    g = model.grounding_tokenizer_input.prepare({k: inp[k] for k in KEYS})
    ctx = inp["context"]
    if case["grounding"] == "null":
        g, ctx = model.grounding_tokenizer_input.get_null_input(), inp["uc"]
    try:
        return model(dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=ctx, inpainting_extra_input=None,
                          grounding_extra_input=inp["sem"] if extra is None else extra, grounding_input=g))
    finally:
        model.first_conv_type = "GLIGEN"


@pytest.mark.parametrize("case", sm.UNET_CASES, ids=[c["name"] for c in sm.UNET_CASES])
def test_tiny_unet_matches_reference_golden(case):
    """12-channel first conv, 16 x 16 latent, 4 tokens, B = 2 against openaimodel_original's output under the bound of
    test_gpu_sp.py::test_tiny_unet_matches_reference_golden (the same engine, first-conv width and token count as its canny cases); graph
    replay == eager bitwise; another class map changes the output on the GLIGEN conv and changes no bit on the SD conv"""
    model = get_model()
    inp, ref = _load(case)
    out = _golden_call(model, case, inp)
    r = report(case["name"], out, ref)
    assert r < 2.1e-3, r
    model.engine.use_graphs = False
    try:
        eager = _golden_call(model, case, inp)
    finally:
        model.engine.use_graphs = True
    assert torch.equal(eager, out), "graph replay == eager"
    assert model.engine.cond["R"] == 0 and model.engine.cond["mo"] == 4
    other = _golden_call(model, case, inp, extra=inp["sem"].flip(-1).contiguous())
    if case["sdconv"]:
        assert torch.equal(other, out), "the SD conv reads the latent alone"
    else:
        d = rel_l2(other, out)
        print(f"[{case['name']}] another class map for the downsampler moves the output by rel_l2 = {d:.2e}")
        assert not torch.equal(other, out), "the GLIGEN conv reads the downsampled map"


def test_cfg_batched_2b_equals_two_calls():
    """[cond ; null] as one 2B batch == two B-sized calls within 1e-6 (test_gpu_sp.py::test_cfg_batched_2b_equals_two_calls); both halves
    read the same extra"""
    model = get_model()
    eng, tok = model.engine, model.tokenizer
    inp, _ = _load(sm.by_name("sem_unet_s1"))
    x = inp["x"].to(DEV)
    objs, null = tok.tokens(inp["sem"], inp["mask"]), tok.null_tokens().expand(2, -1, -1)
    extra = model.downsampler(inp["sem"])
    assert tuple(extra.shape) == (2, 8, 16, 16)

    def one(ctx, o, reps):
        eng.set_conditioning_tokens(ctx, o, 16)
        eng.set_grounding_extra(extra)
        return eng.forward(x, 981.0, 1.0, False, reps).clone()
    ec, eu = one(inp["context"], objs, 1), one(inp["uc"], null, 1)
    e2 = one(torch.cat([inp["context"], inp["uc"]], 0), torch.cat([objs, null], 0), 2)
    rc, ru = rel_l2(e2[:2], ec), rel_l2(e2[2:], eu)
    print(f"[sem 2B] rel_l2 cond {rc:.2e} uncond {ru:.2e}")
    assert rc < 1e-6 and ru < 1e-6, (rc, ru)
    assert rel_l2(ec, eu) > 1e-2


# ------------------------------------------------------------------------------------------- the interface
def _write_sem_checkpoint(path):
    """stubs.write_synthetic_checkpoint's container with the model of a sem checkpoint: the tokenizer / downsampler targets and tensors, no
    ``*.rela_fuse.*`` tensor; the file is not named after the family"""
    ck = stubs.write_synthetic_checkpoint(path, TINY, VAE_TINY, max_relations=10)
    cfg = sm.SEM_TINY
    tok, ds = sm.targets()
    params = ck["config_dict"]["_content"]["model"]["params"]
    params["grounding_tokenizer"] = {"target": tok, "params": {"in_dim": 152, "resize_input": cfg.sp_resize_input, "out_dim": 768}}
    params["grounding_downsampler"] = {"target": ds, "params": {"in_dim": 152, "resize_input": cfg.ds_resize_input, "out_dim": 8}}
    ck["config_dict"]["_content"]["grounding_tokenizer_input"]["target"] = "grounding_input.sem_grounding_tokinzer_input.GroundingNetInput"
    ck["model"] = {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in recipe.state_dict(cfg, 0).items()}
    torch.save(ck, path)
    return ck


def test_interface_on_a_sem_checkpoint(tmp_path):
    """load_all_models, run_one_image, run_batch_images (one map per prompt) and gligen_inference.run at 16 x 16 latents with 4 steps and
    alpha_type [0.5, 0, 0.5] (both first convs run), no phrases and no CLIP model: the latents equal PLMSSampler driven by hand, the map and
    the negative prompt enter, and the refusals"""
    from PIL import Image
    from layoutllm_t2i_amd.model import LatentDiffusion
    from layoutllm_t2i_amd.sampler import PLMSSampler
    p = str(tmp_path / "tiny_gligen_model.pth")
    _write_sem_checkpoint(p)
    with pytest.raises(NotImplementedError, match="strict"):
        itf.load_all_models(p, DEV, strict=True)
    am = itf.load_all_models(p, DEV)
    model, autoencoder, text_encoder = am[0], am[1], am[2]
    assert isinstance(model.grounding_tokenizer_input, SemGroundingNetInput) and model.cfg == dataclasses.replace(sm.SEM_TINY)
    assert model.first_conv_restorable and type(model.tokenizer) is semantic.SemTokenizer and model.downsampler.out_side == 16
    assert model.tokenizer.class_map is model.downsampler.class_map
    img = str(tmp_path / "sem.png")
    Image.fromarray(sm.test_image(), "L").save(img)
    flipped = Image.open(img).transpose(Image.FLIP_LEFT_RIGHT)
    prompt, alpha_type, S = "a living room", [0.5, 0.0, 0.5], 4
    args = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=S)
    meta = dict(prompt=prompt, sem=img, alpha_type=alpha_type)
    torch.manual_seed(123)
    noise = torch.randn(2, 4, 16, 16).to(DEV)
    dec = autoencoder.decode

    def run(fn=itf.run_one_image, meta_=meta, args_=args):
        captured = {}
        autoencoder.decode = lambda lat: dec(captured.setdefault("lat", lat.clone()))
        model.first_conv_type = "GLIGEN"
        try:
            imgs = fn(am, dict(args_), meta_, noise, None, None, device=DEV)
        finally:
            autoencoder.decode = dec
        assert len(imgs) == 2 and imgs[0].size == (32, 32) and imgs[0].mode == "RGB"
        assert model.first_conv_type == "SD", "the scale-0 steps switched to the SD conv"
        return captured["lat"]

    def by_hand(maps, prompts, neg=""):
        """PLMSSampler driven by hand on the batch prepare_batch_sem builds"""
        model.first_conv_type = "GLIGEN"
        batch = itf.prepare_batch_sem({"sem": maps}, 2, DEV)
        sampler = PLMSSampler(am[3], model, alpha_generator_func=partial(itf.alpha_generator, type=alpha_type), set_alpha_scale=itf.set_alpha_scale)
        g = model.grounding_tokenizer_input.prepare(batch, text_encoder)
        inp = dict(x=noise, timesteps=None, context=text_encoder.encode(prompts), relations=None, grounding_input=g,
                   inpainting_extra_input=None, grounding_extra_input=batch["sem"])
        return sampler.sample(S=S, shape=(2, 4, 16, 16), input=inp, uc=text_encoder.encode([neg]).repeat(2, 1, 1), guidance_scale=7.5)
    lat = run()
    assert torch.isfinite(lat).all() and torch.equal(lat, by_hand(img, [prompt] * 2)), "run_one_image == the sampler by hand"
    assert torch.equal(run(), lat), "a second run, cached model"
    d = rel_l2(run(meta_=dict(meta, sem=flipped)), lat)
    print(f"[sem interface] a flipped map moves the latent by rel_l2 = {d:.2e}")
    assert d > 1e-3, "the map enters"
    neg = run(args_=dict(args, negative_prompt="blurry"))
    assert rel_l2(neg, lat) > 1e-3 and torch.equal(neg, by_hand(img, [prompt] * 2, "blurry")), "negative_prompt enters"
    both = run(itf.run_batch_images, dict(prompts=[prompt, "a kitchen"], sem=[img, flipped], alpha_type=alpha_type))
    assert torch.equal(both, by_hand([img, flipped], [prompt, "a kitchen"])), "run_batch_images, one map per prompt == the sampler by hand"
    from layoutllm_t2i_amd import gligen_inference as gi
    gi._MODELS[p] = am
    try:
        n1 = noise[:1].clone()
        out = gi.run(dict(ckpt=p, prompt=prompt, sem=img, alpha_type=alpha_type),
                     dict(batch_size=1, guidance_scale=7.5, no_plms=False, device=DEV, steps=S), starting_noise=n1)
        assert len(out) == 1 and out[0].size == (32, 32)
        model.first_conv_type = "GLIGEN"
        one = itf.run_one_image(am, dict(batch_size=1, no_plms=False, guidance_scale=7.5, steps=S), meta, n1, None, None, device=DEV)
        assert np.array_equal(np.asarray(out[0]), np.asarray(one[0])), "gligen_inference.run == run_one_image"
    finally:
        gi._MODELS.pop(p, None)
    # refusals, before any kernel runs
    a = dict(args)
    with pytest.raises(ValueError, match="canny_image\\) given to a semantic-map checkpoint"):
        itf.run_one_image(am, a, dict(prompt=prompt, canny_image=img), noise, None, None, device=DEV)
    with pytest.raises(ValueError, match=r"meta\['input_image'\]"):
        itf.run_one_image(am, a, dict(meta, input_image=img), noise, None, None, device=DEV)
    with pytest.raises(ValueError, match=r"meta\['images'\]"):
        itf.run_one_image(am, a, dict(meta, images=[img]), noise, None, None, device=DEV)
    with pytest.raises(ValueError, match=r"meta\['locations'\]"):
        itf.run_one_image(am, a, dict(meta, locations=[[0.1, 0.1, 0.4, 0.4]], phrases=["a sofa"]), noise, None, None, device=DEV)
    with pytest.raises(ValueError, match="16 x 16"):
        itf.run_one_image(am, a, meta, torch.randn(2, 4, 16, 24).to(DEV), None, None, device=DEV)
    with pytest.raises(ValueError, match="needs its class map"):
        itf.run_one_image(am, a, dict(prompt=prompt, alpha_type=alpha_type), noise, None, None, device=DEV)
    with pytest.raises(ValueError, match="grounding_extra_input"):
        g = model.grounding_tokenizer_input.prepare(itf.prepare_batch_sem(meta, 2, DEV))
        ctx = torch.zeros(2, 77, 768)
        PLMSSampler(LatentDiffusion(device=DEV), model).sample(S=2, shape=(2, 4, 16, 16),
                                                                input=dict(x=noise, timesteps=None, context=ctx, grounding_input=g), uc=ctx, guidance_scale=7.5)
