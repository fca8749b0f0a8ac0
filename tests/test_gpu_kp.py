"""The keypoint grounding family (``checkpoint_generation_keypoint.pth``) on the GPU: the pose-token input kernel, the fuser's attention at
the key counts N + 17 P in the engine's layout, the tiny UNet against the reference's own outputs (tests/golden/kp_*.npz) in default and
strict mode, batched CFG, the sampler, one full-width level against tests/kp_ref.py, and the interface on a tiny keypoint checkpoint."""
import dataclasses
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import kp_cases as kc
import kp_ref
import stubs
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import ops, recipe, weights
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, UNetConfig
from layoutllm_t2i_amd.model import KeypointGroundingNetInput, LatentDiffusion, UNetModel
from layoutllm_t2i_amd.sampler import PLMSSampler
from layoutllm_t2i_amd.weights import q_fold
from oracle import plms_ref
from test_gpu_attention_layouts import _attn_exp2
from test_gpu_kernels import _attn_ref, check
from test_gpu_model import rel_l2, report
from test_gpu_strict import rel, split
from test_gpu_ti import _engine_layout_launch

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
NAN = float("nan")
KEYS = kp_ref.KEYS
PLMS_TINY_BOUND = 3.1e-3          # tests/test_gpu_model.py / test_gpu_norel.py::test_plms_tiny_matches_reference_golden


def rnd(tag, shape, scale=1.0):
    return T(recipe.normal(f"gpukp.{tag}", tuple(shape), 43)) * scale


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


# ------------------------------------------------------------------------------------------- posnet_input_kp
@pytest.mark.parametrize("P,D", [(3, 768), (1, 64)], ids=["P3-D768", "P1-D64"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_posnet_input_kp(dtype, P, D):
    """the MLP input rows vs the torch expression of keypoint_grounding_net.py:39-56 with the tolerances of
    test_gpu_kernels.py::test_posnet_input_and_timestep_embedding; padded widths 832 and 128, pad columns exactly 0 (the kernel writes them:
    the buffer starts as NaN); NaN sentinels before and behind the output stay NaN; every table row is non-zero and distinct, so a wrong
    t / 17 or t % 17 shows"""
    B, F, tok = 2, 8, 17 * P
    ld = (D + 4 * F + 63) // 64 * 64
    assert ld == {768: 832, 64: 128}[D]
    points = T(np.abs(recipe.uniform(f"gpukp.pts{P}", (B, tok, 2), 3)))
    masks = (T(np.abs(recipe.uniform(f"gpukp.m{P}", (B, tok), 3))) > 0.4).float()
    masks[0, 1], masks[1, tok - 1] = 0.25, 0.5            # a true blend, not a select
    assert 0 < int((masks == 0).sum()) and 0 < int((masks == 1).sum())
    pe, ke = rnd(f"pe{P}.{D}", (P, D), 0.5), rnd(f"ke{D}", (17, D), 0.5)
    assert float(pe.abs().amax(1).min()) > 0 and float(ke.abs().amax(1).min()) > 0
    npn, nxy = rnd(f"np{D}", (D,), 0.5), rnd("nxy", (4 * F,), 0.5)
    n, G = B * tok * ld, 128
    buf = torch.full((2 * G + n,), NAN, dtype=dtype, device=DEV)
    out = buf[G:G + n].view(B, tok, ld)
    d = lambda x: x.to(DEV)
    ops.posnet_input_kp(d(points), d(masks), d(pe), d(ke), d(npn), d(nxy), F, out)
    sd = {"position_net.person_embeddings": pe, "position_net.keypoint_embeddings": ke, "position_net.null_person_feature": npn,
          "position_net.null_xy_feature": nxy}
    want = kp_ref.mlp_input(sd, points, masks, F)
    check(out[..., :D + 4 * F], want, f"posnet_input_kp P{P} D{D} {dtype}")
    h = buf.cpu()
    assert float(h[G:G + n].view(B, tok, ld)[..., D + 4 * F:].float().abs().max()) == 0.0, "pad columns must be written as zeros"
    assert torch.isnan(h[:G]).all() and torch.isnan(h[G + n:]).all(), "sentinel overwritten"


# ------------------------------------------------------------------------------------------- fuser attention at N + 17 P keys
# (d, N, P): Nk = N + 17 P = 21 (7 pad rows), 140, 192 (exactly three key tiles; N = 56 is level 3 of a 56 x 64 latent), 200, 392, 115 (5 pad rows)
FUSER_CASES = [(16, 4, 1), (16, 4, 8), (40, 56, 8), (40, 64, 8), (80, 256, 8), (160, 64, 3)]


@pytest.mark.parametrize("d,N,P", FUSER_CASES, ids=[f"d{c[0]}-N{c[1]}-P{c[2]}" for c in FUSER_CASES])
def test_fuser_attention_at_keypoint_key_counts(d, N, P):
    """single-fp16 and split-fp16 kernels in the engine's layout (rows = N + 17 P rounded up to 8 per sample, NaN pad rows and NaN behind key
    Nk) with the tolerances of tests/test_gpu_ti.py::test_fuser_attention_at_text_image_key_counts: rtol 2e-3 / atol 2e-4 vs fp32 on the same
    fp16 operands; rel-L2 < 1e-6 vs fp64 of hi + lo, the single-fp16 kernel > 20 x worse"""
    B, H = 2, 2
    ng = 17 * P
    C, Nk, rows = H * d, N + ng, N + ((ng + 7) & ~7)
    assert (Nk, rows - Nk) == {(4, 1): (21, 7), (4, 8): (140, 0), (56, 8): (192, 0), (64, 8): (200, 0), (256, 8): (392, 0), (64, 3): (115, 5)}[(N, P)]
    q, k, v = rnd(f"q{d}.{N}.{P}", (B, N, C)) * 1.2, rnd(f"k{d}.{N}.{P}", (B, Nk, C)) * 1.2, rnd(f"v{d}.{N}.{P}", (B, Nk, C))
    k[:, Nk - 3] = 3.0 * q[:, 1]                         # a dominant key among the last person's tokens (the last key tile)
    (qh, ql), (kh, kl), (vh, vl) = split(q * q_fold(d)), split(k), split(v)
    o1 = _engine_layout_launch(qh, None, kh, None, vh, None, B, H, d, N, Nk, rows, False)
    check(o1, _attn_ref(qh.float() / q_fold(d), kh.float(), vh.float(), H), f"fuser attn f16 d{d} N{N} Nk{Nk}", rtol=2e-3, atol=2e-4)
    o2 = _engine_layout_launch(qh, ql, kh, kl, vh, vl, B, H, d, N, Nk, rows, True)
    f64 = lambda hi, lo: hi.double() + lo.double()
    want = _attn_exp2(f64(qh, ql), f64(kh, kl), f64(vh, vl), H)
    r, r1 = rel(o2[..., :C].double() + o2[..., C:].double(), want), rel(o1, want)
    print(f"[kp fuser attn split d={d} N={N} Nk={Nk}] rel_l2 = {r:.2e} (single-fp16 kernel {r1:.2e})")
    assert r < 1e-6 and r1 > 20 * r, (r, r1)


# ------------------------------------------------------------------------------------------- whole model: tiny UNet vs the reference
_models = {}


def get_model(P, split_weights=False):
    key = (P, split_weights)
    if key not in _models:
        base = kc.KP_TINY[P]
        m = UNetModel(dataclasses.replace(base, split_weights=split_weights), recipe.state_dict(base, 0), device=DEV,
                      sd_first_conv=recipe.sd_first_conv(base, 0))
        m.grounding_tokenizer_input = KeypointGroundingNetInput()
        _models[key] = m
    return _models[key]


def _golden_call(model, case, inp, **override):
    """the upstream ``input`` dict: no "relations" key"""
    model.fuser_scale = case["scale"]
    model.first_conv_type = "SD" if case["sdconv"] else "GLIGEN"
    g = model.grounding_tokenizer_input.prepare({**{k: inp[k] for k in KEYS}, **override})
    if case["grounding"] == "null":
        g = model.grounding_tokenizer_input.get_null_input()
    try:
        return model(dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"],
                          inpainting_extra_input=None, grounding_extra_input=None, grounding_input=g))
    finally:
        model.first_conv_type = "GLIGEN"


def _load(case):
    return {a: T(v) for a, v in kc.case_inputs(case).items()}, T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"])


@pytest.mark.parametrize("case", kc.UNET_CASES, ids=[c["name"] for c in kc.UNET_CASES])
def test_tiny_unet_matches_reference_golden(case):
    """default mode, the bound of test_gpu_model.py / test_gpu_ti.py::test_tiny_unet_matches_reference_golden; graph replay == eager bitwise"""
    model = get_model(case["P"])
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
    assert model.engine.cond["R"] == 0 and model.engine.cond["mo"] == 17 * case["P"]


@pytest.mark.parametrize("case", kc.UNET_CASES, ids=[c["name"] for c in kc.UNET_CASES])
def test_tiny_unet_strict_matches_reference_golden(case):
    """strict mode on a split_weights handle, the bounds of test_gpu_ti.py::test_tiny_unet_strict_matches_reference_golden"""
    model = get_model(case["P"], True)
    inp, ref = _load(case)
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


@pytest.mark.parametrize("P", [3, 8])
def test_lazy_strict_hoists_keep_points_and_masks(P):
    """a split handle conditioned in DEFAULT mode keeps device copies of points and masks and computes the strict hoists with the first strict
    forward: the bits of conditioning in strict mode, within the strict bounds of the golden; other points and masks in between change them"""
    case = kc.by_name(f"kp_unet_tiny_p{P}_s1")
    model = get_model(P, True)
    eng = model.engine
    inp, ref = _load(case)
    x = inp["x"].to(DEV)
    model.set_strict(False)
    eng.set_conditioning_kp(inp["context"], inp["points"], inp["masks"], 16)
    eng.forward(x, 981.0, 1.0, False, 1)
    try:
        eng.set_option(50, 1)
        lazy = eng.forward(x, 981.0, 1.0, False, 1).clone()
        r = report(f"{case['name']} lazy strict", lazy, ref)
        outside = float(((lazy.cpu() - ref).abs() > 1e-4 + 1e-3 * ref.abs()).float().mean())
        assert r < 5e-5 and outside < 0.01, (r, outside)
        eng.set_conditioning_kp(inp["context"], inp["points"], inp["masks"], 16)
        assert torch.equal(eng.forward(x, 981.0, 1.0, False, 1), lazy), "lazy hoists == hoists at conditioning time"
        eng.set_option(50, 0)
        pts2, m2 = inp["points"].flip(1).contiguous(), inp["masks"].flip(1).contiguous() * 0.75
        eng.set_conditioning_kp(inp["context"], pts2, m2, 16)
        eng.set_option(50, 1)
        lazy2 = eng.forward(x, 981.0, 1.0, False, 1).clone()
        eng.set_conditioning_kp(inp["context"], pts2, m2, 16)
        assert torch.equal(eng.forward(x, 981.0, 1.0, False, 1), lazy2)
        assert rel_l2(lazy2, lazy) > 1e-3
    finally:
        eng.set_option(50, 0)
        model.set_strict(False)


# ------------------------------------------------------------------------------------------- grounding actually enters
def test_zeroed_masks_give_the_null_grounding_golden():
    case, null_case = kc.by_name("kp_unet_tiny_p8_s1"), kc.by_name("kp_unet_tiny_null")
    model = get_model(8)
    inp, ref = _load(case)
    _, null_ref = _load(null_case)
    out = _golden_call(model, case, inp)
    zeroed = _golden_call(model, case, inp, masks=torch.zeros_like(inp["masks"]))      # the points stay: a zero mask blends them away
    moved = rel_l2(zeroed, out)
    r = report("kp_unet_tiny_p8_s1 masks zeroed vs null golden", zeroed, null_ref)
    print(f"[kp_unet_tiny_p8_s1] masks zeroed: moved by rel_l2 = {moved:.3e}")
    assert moved > 1e-2, moved
    assert r < 2.1e-3, r


# ------------------------------------------------------------------------------------------- batched CFG
def test_cfg_batched_2b_equals_two_calls():
    """[cond ; null] as one 2B batch == two B-sized calls within 1e-6, as tests/test_gpu_ti.py::test_cfg_batched_2b_equals_two_calls asserts"""
    eng = get_model(8).engine
    inp, _ = _load(kc.by_name("kp_unet_tiny_p8_s1"))
    x, z, cat = inp["x"].to(DEV), torch.zeros_like, (lambda a, b: torch.cat([a, b], 0))
    eng.set_conditioning_kp(inp["context"], inp["points"], inp["masks"], 16)
    ec = eng.forward(x, 981.0, 1.0, False, 1).clone()
    eng.set_conditioning_kp(inp["uc"], z(inp["points"]), z(inp["masks"]), 16)
    eu = eng.forward(x, 981.0, 1.0, False, 1).clone()
    eng.set_conditioning_kp(cat(inp["context"], inp["uc"]), cat(inp["points"], z(inp["points"])), cat(inp["masks"], z(inp["masks"])), 16)
    e2 = eng.forward(x, 981.0, 1.0, False, 2).clone()
    rc, ru = rel_l2(e2[:2], ec), rel_l2(e2[2:], eu)
    print(f"[kp 2B] rel_l2 cond {rc:.2e} uncond {ru:.2e}")
    assert rc < 1e-6 and ru < 1e-6, (rc, ru)
    assert rel_l2(ec, eu) > 1e-2                        # the two halves are different problems


def test_engine_refuses_the_other_families_inputs():
    from layoutllm_t2i_amd import _lib
    eng = get_model(8).engine
    inp, _ = _load(kc.by_name("kp_unet_tiny_p8_s1"))
    with pytest.raises(ValueError, match="points and masks"):
        eng.set_conditioning(inp["context"], None, torch.zeros(2, 136, 4), inp["masks"], torch.zeros(2, 136, 768), 16)
    with pytest.raises(ValueError, match="8 persons"):
        eng.set_conditioning_kp(inp["context"], inp["points"][:, :51], inp["masks"][:, :51], 16)
    d = lambda t: t.to(DEV).contiguous()
    keep = [d(inp["context"]), d(torch.zeros(2, 136, 4)), d(inp["masks"]), d(torch.zeros(2, 136, 768))]
    rc = eng._lib.gl_set_conditioning(eng.handle, keep[0].data_ptr(), None, keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), 2, 77, 0, 16, None)
    assert rc == -1 and "grounding = 2 (keypoint)" in _lib.last_error(eng.handle)


# ------------------------------------------------------------------------------------------- sampler
def test_plms_4_steps_vs_the_oracle_sampler():
    """4 PLMS steps, CFG 7.5, alpha ramp [0.5, 0, 0.5] (scale 1, 1, 0, 0: the fuser switches off and the first conv switches to the SD one),
    B = 2, P = 3, through PLMSSampler with the upstream input dict, against oracle.plms_ref driven by tests/kp_ref.py"""
    P, S, alpha_type, guidance = 3, 4, [0.5, 0.0, 0.5], 7.5
    cfg = kc.KP_TINY[P]
    case = kc.by_name("kp_unet_tiny_p3_s1")
    inp, _ = _load(case)
    assert 0.0 in [float(a) for a in itf.alpha_generator(S, alpha_type)]
    model = get_model(P)
    model.first_conv_type = "GLIGEN"
    sampler = PLMSSampler(LatentDiffusion(device=DEV), model, alpha_generator_func=partial(itf.alpha_generator, type=alpha_type),
                          set_alpha_scale=itf.set_alpha_scale)
    g = model.grounding_tokenizer_input.prepare({k: inp[k] for k in KEYS}, None)
    d = dict(x=inp["x"].to(DEV), timesteps=None, context=inp["context"], grounding_input=g, inpainting_extra_input=None, grounding_extra_input=None)
    try:
        out = sampler.sample(S=S, shape=tuple(inp["x"].shape), input=d, uc=inp["uc"], guidance_scale=guidance)
        assert model.first_conv_type == "SD", "restore_first_conv_from_SD must stick (openaimodel.py:393-411)"
    finally:
        model.first_conv_type = "GLIGEN"
        model.fuser_scale = 1.0
    sd = {k: T(np.asarray(v)).float() for k, v in recipe.state_dict(cfg, 0).items()}
    fc = {k: T(v) for k, v in recipe.sd_first_conv(cfg, 0).items()}
    with torch.no_grad():
        ref = plms_ref.plms_sample(kp_ref.make_eps_fn(sd, cfg, inp, guidance, fc), inp["x"], S, alpha_type)
    r = report("kp_plms_tiny_4", out, ref)
    assert r < PLMS_TINY_BOUND, r


# ------------------------------------------------------------------------------------------- one full-width level
def test_default_mode_full_width_level_vs_kp_ref():
    """model_channels 320, 8 heads, ONE level of width 1280 (d = 160) on an 8 x 8 latent (N = 64), P = 8 (Nk = 200), [cond ; null] with one
    latent (2B = 2), default mode, against tests/kp_ref.py on the same fp16-representable weights: the bound and the method of
    tests/test_gpu_ti.py::test_default_mode_full_width_level_vs_ti_ref (weights drawn on the device, as tests/test_gpu_norel.py does)"""
    cfg = kc.kp_cfg(UNetConfig(image_size=8, model_channels=320, channel_mult=(4,), attention_resolutions=(1,), num_res_blocks=1), 8)
    sd = {k: (v.half().float() if v.dim() >= 2 else v) for k, v in weights.random_state_dict(cfg, DEV, seed=3).items()}
    model = UNetModel(cfg, sd, device=DEV)
    assert {l.d_head for l in model.engine.plan.st_layers()} == {160} and {l.cin for l in model.engine.plan.st_layers()} == {1280}
    inp = {k: T(v) for k, v in recipe.synth_inputs_kp(cfg, 1, 8, seed=4321).items()}
    h16 = lambda t: t.half().float()
    g = {k: inp[k] for k in KEYS}
    gn = kp_ref.null_grounding(g)
    cat = lambda a, b: torch.cat([a, b], 0)
    model.engine.set_conditioning_kp(cat(inp["context"], inp["uc"]), cat(g["points"], gn["points"]), cat(g["masks"], gn["masks"]), 8)
    out = model.engine.forward(h16(inp["x"]).to(DEV), 481.0, 1.0, False, 2).clone()
    t = torch.full((1,), 481, dtype=torch.long)
    osd = {k: v.cpu() for k, v in sd.items()}
    with torch.no_grad():
        torch.set_num_threads(min(16, max(1, os.cpu_count() or 1)))
        rc = kp_ref.unet_forward(osd, cfg, h16(inp["x"]), t, h16(inp["context"]), g)
        ru = kp_ref.unet_forward(osd, cfg, h16(inp["x"]), t, h16(inp["uc"]), gn)
    r = report("kp L2_c1280_d160_8x8_P8", out, cat(rc, ru))
    assert r < 7.5e-4, r
    del model
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- the interface
def _write_kp_checkpoint(path, P):
    """stubs.write_synthetic_checkpoint's container with the model of a keypoint checkpoint: keypoint PositionNet target and tensors, no
    ``*.rela_fuse.*`` tensor, the keypoint grounding-tokenizer input"""
    ck = stubs.write_synthetic_checkpoint(path, TINY, VAE_TINY, max_relations=10)
    content = ck["config_dict"]["_content"]
    content["model"]["params"]["grounding_tokenizer"] = {"target": kc.KP_TARGET, "params": {"max_persons_per_image": P, "out_dim": 768}}
    content["grounding_tokenizer_input"]["target"] = "grounding_input.keypoint_grounding_tokinzer_input.GroundingNetInput"
    ck["model"] = {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in recipe.state_dict(kc.KP_TINY[P], 0).items()}
    torch.save(ck, path)


def test_run_one_image_on_a_keypoint_checkpoint(tmp_path):
    """run_one_image with the stub text encoder, no CLIP model, no phrases: the latent equals the oracle pipeline (kp_ref under
    oracle.plms_ref on the conditioning restated on the CPU) within the bound of test_boundary.py::test_run_batch_images_equals_the_oracle_
    pipeline; a second run on the cached model is identical; gligen_inference.run routes the same way"""
    P = 3
    cfg = kc.KP_TINY[P]
    p = str(tmp_path / "tiny_gligen_keypoint.pth")
    _write_kp_checkpoint(p, P)
    am = itf.load_all_models(p, DEV)
    model, autoencoder, text_encoder, diffusion, config = am
    assert isinstance(model.grounding_tokenizer_input, KeypointGroundingNetInput) and model.cfg.grounding == "keypoint"
    assert model.cfg.max_persons == P and model.cfg.relation is False
    z = np.load(os.path.join(GOLD, "kp_prepare_batch.npz"))
    locations = z["locations"].tolist()
    prompt, alpha_type, S = "A young man and a small boy are talking", [0.5, 0.0, 0.5], 4
    torch.manual_seed(123)
    noise = torch.randn(2, 4, 16, 16)
    args = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=S)
    meta = dict(prompt=prompt, locations=locations, alpha_type=alpha_type)
    dec = autoencoder.decode

    def run():
        captured = {}
        autoencoder.decode = lambda lat: dec(captured.setdefault("lat", lat.clone()))
        model.first_conv_type = "GLIGEN"
        try:
            imgs = itf.run_one_image(am, dict(args), meta, noise.to(DEV), None, None, device=DEV)
        finally:
            autoencoder.decode = dec
        assert len(imgs) == 2 and imgs[0].size == (32, 32) and imgs[0].mode == "RGB"
        return captured["lat"]
    lat = run()
    enc = text_encoder.to("cpu")
    batch = itf.prepare_batch_kp(meta, 2, P)
    cond = dict(context=enc.encode([prompt] * 2), uc=enc.encode([""]).repeat(2, 1, 1), **batch)
    text_encoder.to(DEV)
    assert float(cond["masks"][0].sum()) == 19.0
    sd = {k: T(np.asarray(v)).float() for k, v in recipe.state_dict(cfg, 0).items()}
    fc = {k: T(v) for k, v in recipe.sd_first_conv(cfg, 0).items()}
    with torch.no_grad():
        lat_ref = plms_ref.plms_sample(kp_ref.make_eps_fn(sd, cfg, cond, 7.5, fc), noise, S, alpha_type)
    rl = rel_l2(lat, lat_ref)
    print(f"[kp interface] latent rel_l2 = {rl:.3e}")
    assert rl < 2.7e-3, rl
    assert torch.equal(run(), lat), "a second run on the cached model"
    # a rectangular latent, the batch entry with one pose layout per prompt, and gligen_inference.run without CLIP objects
    model.first_conv_type = "GLIGEN"
    rect = itf.run_batch_images(am, dict(args), dict(prompts=[prompt, "two people"], locations=[locations, locations[:1]], alpha_type=alpha_type),
                                torch.randn(2, 4, 16, 24).to(DEV), None, None, device=DEV)
    assert len(rect) == 2 and rect[0].size == (48, 32)
    from layoutllm_t2i_amd import gligen_inference as gi
    gi._MODELS[p] = am
    try:
        out = gi.run(dict(ckpt=p, prompt=prompt, locations=locations, alpha_type=alpha_type),
                     dict(batch_size=1, guidance_scale=7.5, no_plms=False, device=DEV, steps=S), starting_noise=torch.randn(1, 4, 16, 16).to(DEV))
    finally:
        gi._MODELS.pop(p, None)
    assert len(out) == 1 and out[0].size == (32, 32)
    with pytest.raises(ValueError, match="4 persons"):
        itf.run_one_image(am, dict(args), dict(meta, locations=[locations[0]] * 4), noise.to(DEV), None, None, device=DEV)
