"""Grounded inpainting on a real MI355X: the asymmetric-pad downsample conv, the posterior and latent-blend kernels, the VAE
encoder engine (vs the reference golden, the fp32 mirror and its own op-level sequence) and the masked PLMS sampler (vs an
oracle loop fed the engine's eps, vs the reference golden), then the interface end to end on a synthetic checkpoint."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import golden_cases as gc
import stubs
import vae_encoder_pyref
from layoutllm_t2i_amd import _lib, host, ops, recipe
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, VAEConfig
from layoutllm_t2i_amd.interface import denoise
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel
from layoutllm_t2i_amd.vae import VAEDecoder, VAEEncoder
from oracle import plms_ref

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def enc_sd(cfg):
    return {**recipe.vae_state_dict(cfg, 0), **recipe.vae_encoder_state_dict(cfg, 0)}


# ------------------------------------------------------------------------------------------- kernels
PAD01 = [(1, 128, 128, 512), (1, 256, 256, 256), (1, 512, 512, 128),       # the real encoder's three downsamples
         (2, 64, 64, 96), (2, 192, 128, 40), (3, 512, 256, 24), (1, 320, 64, 20)]


@pytest.mark.parametrize("opts", [(), ((30, 0),), ((13, 0),)], ids=["default", "no8wave", "nokslice"])
@pytest.mark.parametrize("B,Cin,Cout,side", PAD01)
def test_conv3x3_pad01_matches_padded_conv(B, Cin, Cout, side, opts):
    init_device()
    x = T(recipe.normal(f"inp.pad01.x.{Cin}.{side}", (B, Cin, side, side), 3)).half().float()
    w = (T(recipe.normal(f"inp.pad01.w.{Cin}.{Cout}", (Cout, Cin, 3, 3), 3)) * np.float32((9 * Cin) ** -0.5)).half().float()
    b = T(recipe.normal(f"inp.pad01.b.{Cout}", (Cout,), 3))
    with torch.no_grad():
        torch.set_num_threads(16)
        ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)                       # model.py:74-76
    from layoutllm_t2i_amd.weights import pack_conv3x3
    xd = x.permute(0, 2, 3, 1).reshape(B * side * side, Cin).half().to(DEV).contiguous()
    out = torch.empty(B * (side // 2) ** 2, Cout, dtype=torch.float16, device=DEV)
    try:
        for k, v in opts:
            ops.set_option(k, v)
        ops.conv3x3_pad01(xd, pack_conv3x3(w.to(DEV)), out, B, side, side, b.to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.set_option(30, 1)
        ops.set_option(13, 3)
    got = out.float().cpu().reshape(B, side // 2, side // 2, Cout).permute(0, 3, 1, 2)
    r = rel_l2(got, ref)
    err = float((got - ref).abs().max())
    assert r < 1e-3 and err < 1e-2 * float(ref.abs().max()), (r, err)


def test_conv3x3_pad01_rejects_other_geometries():
    init_device()
    x = torch.zeros(64, 64, dtype=torch.float16, device=DEV)
    w = torch.zeros(64, 9 * 64, dtype=torch.float16, device=DEV)
    out = torch.zeros(64, 64, dtype=torch.float16, device=DEV)
    a = _lib.ConvArgs()
    a.inp, a.B, a.Hin, a.Win, a.Cin, a.Hout, a.Wout, a.stride = x.data_ptr(), 1, 8, 8, 64, 4, 4, 1      # stride 1
    a.g.w, a.g.N, a.g.out, a.g.ldc = w.data_ptr(), 64, out.data_ptr(), 64
    import ctypes as C
    assert _lib.lib().gl_conv3x3_pad01(C.byref(a), None) == -1
    a.stride, a.upsample2x = 2, 1
    assert _lib.lib().gl_conv3x3_pad01(C.byref(a), None) == -1
    a.upsample2x, a.in_split = 0, 2
    assert _lib.lib().gl_conv3x3_pad01(C.byref(a), None) == -1


def test_posterior_matches_torch_expression():
    init_device()
    B, E, s = 2, 4, 12
    h = T(recipe.normal("inp.post.h", (B, 2 * E, s, s), 3)) * 3
    w = T(recipe.normal("inp.post.w", (2 * E, 2 * E), 3))
    b = T(recipe.normal("inp.post.b", (2 * E,), 3))
    b[E] += 40.0            # a logvar channel above the clamp
    b[E + 1] -= 50.0        # and one below it
    noise = T(recipe.normal("inp.post.n", (B, E, s, s), 3))
    z, mean = torch.empty(B, E, s, s, device=DEV), torch.empty(B, E, s, s, device=DEV)
    ops.vae_posterior(h.to(DEV), w.to(DEV), b.to(DEV), noise.to(DEV), 0.18215, z, mean)
    mom = F.conv2d(h.double(), w.double().view(2 * E, 2 * E, 1, 1), b.double())
    rm, lv = torch.chunk(mom, 2, dim=1)
    rz = (rm + torch.exp(0.5 * torch.clamp(lv, -30.0, 20.0)) * noise.double()) * 0.18215
    assert rel_l2(mean, rm) < 1e-6 and rel_l2(z, rz) < 1e-6, (rel_l2(mean, rm), rel_l2(z, rz))
    assert torch.allclose(z.double().cpu(), rz, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("side", [16, 15])
@pytest.mark.parametrize("b0,bm", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_latent_blend_is_bitwise_the_torch_expression(b0, bm, side):
    init_device()
    B = 3
    x = T(recipe.normal("inp.bl.x", (B, 4, side, side), 3)).to(DEV)
    x0 = T(recipe.normal("inp.bl.x0", (b0, 4, side, side), 3)).to(DEV)
    n = T(recipe.normal("inp.bl.n", (b0, 4, side, side), 3)).to(DEV)
    mask = host.draw_masks_from_boxes(np.array([[[0.1, 0.2, 0.6, 0.7]], [[0.5, 0.0, 1.0, 0.5]], [[0.0, 0.0, 0.0, 0.0]]])[:bm], side)
    mask = mask.to(DEV)
    mask[:, :, 0, :] = 0.25                                          # a fractional row too
    d = LatentDiffusion(device=DEV)
    t = torch.full((B,), 721, dtype=torch.long, device=DEV)
    a = d.sqrt_alphas_cumprod.gather(-1, t).reshape(B, 1, 1, 1)
    s = d.sqrt_one_minus_alphas_cumprod.gather(-1, t).reshape(B, 1, 1, 1)
    ref = (a * x0 + s * n) * mask + (1.0 - mask) * x                 # ldm.py:19-22, plms.py:98
    got = x.clone()
    ops.latent_blend(got, x0, n, mask, float(d.sqrt_alphas_cumprod[721]), float(d.sqrt_one_minus_alphas_cumprod[721]))
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert torch.equal(got, d.q_sample(x0, t, n) * mask + (1.0 - mask) * x)


# ------------------------------------------------------------------------------------------- encoder engine
def test_tiny_encoder_matches_reference_golden():
    g = np.load(os.path.join(GOLD, "vae_enc_tiny.npz"))
    enc = VAEEncoder(enc_sd(VAE_TINY), VAE_TINY, DEV)
    z = enc.encode(T(g["x"]), T(g["noise"]))
    _, mean = enc.encode_oplevel(T(g["x"]), T(g["noise"]), return_mean=True)
    assert z.shape == g["z"].shape and z.dtype == torch.float32 and torch.isfinite(z).all()
    rz, rm = rel_l2(z, T(g["z"])), rel_l2(mean, T(g["mean"]))
    print(f"[vae_enc_tiny] rel_l2 z={rz:.3e} mean={rm:.3e}")
    assert rz < 6e-3 and rm < 6e-3, (rz, rm)


def test_full_size_encoder_vs_fp32_mirror():
    cfg = VAEConfig()
    sd = enc_sd(cfg)
    x = T(np.clip(recipe.normal("inp.encfull.x", (1, 3, 512, 512), 9) * np.float32(0.5), -1, 1))
    noise = T(recipe.normal("inp.encfull.n", (1, 4, 64, 64), 9))
    enc = VAEEncoder(sd, cfg, DEV)
    z = enc.encode(x, noise)
    osd = {k: (T(np.asarray(v)).half().float() if np.asarray(v).ndim >= 2 else T(np.asarray(v))) for k, v in sd.items()}
    osd["quant_conv.weight"] = T(np.asarray(sd["quant_conv.weight"]))          # applied in fp32 by the engine
    with torch.no_grad():
        torch.set_num_threads(16)
        ref, _ = vae_encoder_pyref.encode(osd, x, cfg.ch_mult, cfg.num_res_blocks, noise, cfg.scale_factor)
    r = rel_l2(z, ref)
    print(f"[vae_enc_full] rel_l2={r:.3e} max|err|={float((z.cpu() - ref).abs().max()):.3e}")
    assert z.shape == (1, 4, 64, 64) and torch.isfinite(z).all() and r < 6e-3, r
    assert torch.equal(z, enc.encode(x, noise))


@pytest.mark.parametrize("cfgname,B,side", [("tiny", 2, 32), ("tiny", 3, 16), ("full", 2, 256), ("full", 1, 768)])
def test_c_encoder_equals_python_op_sequence_bitwise(cfgname, B, side):
    """gl_vae_encode (plan + pool + hipGraph) against encode_oplevel: eager, captured and replayed, two keys on one handle."""
    cfg = VAE_TINY if cfgname == "tiny" else VAEConfig()
    enc = VAEEncoder(enc_sd(cfg), cfg, DEV)
    f = 2 ** (len(cfg.ch_mult) - 1)
    x = T(np.clip(recipe.normal(f"inp.encc.{B}.{side}", (B, 3, side, side), 3) * np.float32(0.5), -1, 1))
    noise = T(recipe.normal(f"inp.encc.n.{B}.{side}", (B, cfg.embed_dim, side // f, side // f), 3))
    ref = enc.encode_oplevel(x, noise)
    enc.use_graphs = False
    eager = enc.encode(x, noise)
    enc.use_graphs = True
    first = enc.encode(x, noise)
    replay = enc.encode(x, noise)
    assert torch.isfinite(ref).all()
    assert torch.equal(eager, ref) and torch.equal(first, ref) and torch.equal(replay, ref)
    x1, n1 = x[:1].contiguous(), noise[:1].contiguous()
    assert torch.equal(enc.encode(x1, n1), enc.encode_oplevel(x1, n1))
    assert torch.equal(enc.encode(x, noise), ref)
    assert _lib.lib().gl_vae_num_launches(enc.handle) > 20


def test_encoder_contract_and_errors():
    cfg = VAE_TINY
    dec = VAEDecoder(enc_sd(cfg), cfg, DEV)
    x = T(np.clip(recipe.normal("inp.ctr.x", (1, 3, 16, 16), 3), -1, 1))
    torch.manual_seed(3)
    z = dec.encode(x)                                               # noise: torch.randn(mean.shape) on the CPU generator
    torch.manual_seed(3)
    assert torch.equal(z, dec.encoder.encode(x, torch.randn(1, 4, 8, 8)))
    assert set(dec.W) == {n for n, *_ in _lib.vae_weight_table(dec.handle)[0]}     # W stays decoder-only
    import ctypes as C
    o = torch.empty(1, 3, 16, 16, device=DEV)
    zz = torch.zeros(1, 4, 8, 8, device=DEV)
    assert _lib.lib().gl_vae_decode(C.c_void_p(dec.encoder.handle), zz.data_ptr(), 1, 8, o.data_ptr(), 0, None) == -1
    assert _lib.lib().gl_vae_encode(C.c_void_p(dec.handle), o.data_ptr(), 1, 16, zz.data_ptr(), zz.data_ptr(), 0, None) == -1
    for bad in ((1, 3, 13, 13), (1, 3, 1024, 1024), (1, 4, 16, 16)):
        with pytest.raises(ValueError):
            dec.encode(torch.zeros(bad))
    only_dec = VAEDecoder(recipe.vae_state_dict(cfg, 0), cfg, DEV)
    with pytest.raises(RuntimeError, match="encoder tensors"):
        only_dec.encode(x)
    with pytest.raises(RuntimeError, match="encoder"):
        VAEDecoder.from_packed(only_dec.W, cfg, DEV).encode(x)
    with pytest.raises(NotImplementedError):
        VAEDecoder({**enc_sd(cfg), "encoder.down.0.attn.0.q.weight": np.zeros((64, 64, 1, 1), np.float32)}, cfg, DEV)


# ------------------------------------------------------------------------------------------- masked sampler
_models = {}


def get_model(strict):
    if strict not in _models:
        import dataclasses
        cfg = dataclasses.replace(TINY, split_weights=True) if strict else TINY
        m = UNetModel(cfg, recipe.state_dict(TINY, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(TINY, 0))
        if strict:
            m.set_strict(True)
        m.grounding_tokenizer_input = GroundingNetInput()
        _models[strict] = m
    return _models[strict]


def plms_case():
    case = next(c for c in gc.CASES if c["name"] == "plms_tiny")
    inp = {a: T(v) for a, v in gc.case_inputs(case).items()}
    g = np.load(os.path.join(GOLD, "plms_inpaint_tiny.npz"))
    return case, inp, g


def run_masked(model, case, inp, mask, x0, steps=None):
    model.first_conv_type = "GLIGEN"
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
    return denoise((model, None, None, LatentDiffusion(device=DEV), {}), inp["context"], inp["uc"], inp["relations"], batch,
                   inp["x"].to(DEV), case["alpha_type"], case["guidance"], steps=steps or case["S"], mask=mask, x0=x0)


class RecordRandnLike:
    """torch.randn_like stand-in that records every draw's shape and value (or replays recorded values)."""
    def __init__(self, replay=None):
        self.shapes, self.values, self.replay, self.real = [], [], replay, torch.randn_like

    def __call__(self, t, *a, **k):
        self.shapes.append(list(t.shape))
        if self.replay is not None:
            v = T(self.replay[len(self.shapes) - 1]).to(t.device, t.dtype)
        else:
            v = self.real(t, *a, **k)
        self.values.append(v.clone())
        return v

    def __enter__(self):
        torch.randn_like = self
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.real


def masked_oracle_loop(eps_fn, x, S, alpha_type, x0, mask, q_noises, diffusion):
    """plms_ref.plms_sample's loop (plms.py:80-163, sigma = 0) with the blend of plms.py:95-99 at the top of every step:
    x = q_sample(x0, t) * mask + (1 - mask) * x, q_sample from the fp32 buffers (ldm.py:19-22), on the device like the reference."""
    sched = plms_ref.make_schedule(S)
    time_range = np.flip(sched["ddim_timesteps"])
    total = len(time_range)
    alphas = plms_ref.alpha_generator(total, alpha_type)
    b = x.shape[0]
    old = []

    def x_prev_of(xc, e, index):
        a_t, a_prev = np.float32(sched["ddim_alphas"][index]), np.float32(sched["ddim_alphas_prev"][index])
        s1m = torch.full((b, 1, 1, 1), float(np.float32(sched["ddim_sqrt_one_minus_alphas"][index])))
        pred_x0 = (xc - s1m * e) / torch.full((b, 1, 1, 1), float(np.sqrt(a_t)))
        dir_xt = torch.full((b, 1, 1, 1), float(np.sqrt(np.float32(1.0) - a_prev))) * e
        return torch.full((b, 1, 1, 1), float(np.sqrt(a_prev))) * pred_x0 + dir_xt

    for i, step in enumerate(time_range):
        index = total - i - 1
        t = torch.full((b,), int(step), dtype=torch.long, device=DEV)
        x = (diffusion.q_sample(x0, t, q_noises[i]) * mask + (1.0 - mask) * x.to(DEV)).cpu()
        t_next = torch.full((b,), int(time_range[min(i + 1, total - 1)]), dtype=torch.long)
        e_t = eps_fn(x, t.cpu(), i, alphas[i])
        if len(old) == 0:
            e_prime = (e_t + eps_fn(x_prev_of(x, e_t, index), t_next, i, alphas[i])) / 2
        elif len(old) == 1:
            e_prime = (3 * e_t - old[-1]) / 2
        elif len(old) == 2:
            e_prime = (23 * e_t - 16 * old[-1] + 5 * old[-2]) / 12
        else:
            e_prime = (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
        x = x_prev_of(x, e_prime, index)
        old.append(e_t)
        if len(old) >= 4:
            old.pop(0)
    return x


@pytest.mark.parametrize("x0_batch", [1, 2])
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
def test_masked_sampler_equals_oracle_loop_given_engine_eps(strict, x0_batch):
    case, inp, g = plms_case()
    model = get_model(strict)
    mask = host.draw_masks_from_boxes(inp["boxes"], case["hw"]).to(DEV)
    x0 = T(g["x0"]).repeat(x0_batch, 1, 1, 1).to(DEV)
    if x0_batch == 2:
        x0[1] *= -0.5
    torch.manual_seed(11)
    with RecordRandnLike() as rec:
        out = run_masked(model, case, inp, mask, x0).cpu()
    want = [[x0_batch] + s[1:] if s[0] == 1 else s for s in g["draw_shapes"].tolist()]     # one x0-shaped draw, then the step's
    assert rec.shapes == want
    q_noises = [rec.values[j] for j in range(len(rec.values)) if j == 0 or (j >= 3 and (j - 3) % 2 == 0)]
    assert len(q_noises) == case["S"] and all(list(n.shape) == list(x0.shape) for n in q_noises)
    eng = model.engine
    z = torch.zeros_like
    cat = lambda a, b: torch.cat([a, b], 0)
    eng.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
                         cat(inp["masks"], z(inp["masks"])), cat(inp["positive_embeddings"], z(inp["positive_embeddings"])), 16)
    state = dict(sd=False)

    def eps_fn(x, t, i, alpha):
        if alpha == 0:
            state["sd"] = True
        e2 = eng.forward(x.to(DEV), float(t[0]), float(alpha), state["sd"], 2).cpu()
        return e2[2:] + case["guidance"] * (e2[:2] - e2[2:])
    ref = masked_oracle_loop(eps_fn, inp["x"], case["S"], case["alpha_type"], x0, mask, q_noises, LatentDiffusion(device=DEV))
    assert torch.equal(out, ref), float((out - ref).abs().max())
    # an all-zero mask regenerates everything: exactly the unmasked run under the same seed (whose draws are the step's only)
    torch.manual_seed(11)
    allz = run_masked(model, case, inp, torch.zeros_like(mask), x0).cpu()
    torch.manual_seed(11)
    un = run_masked(model, case, inp, None, None).cpu()
    assert torch.equal(allz, un)


def test_masked_sampler_matches_reference_golden():
    case, inp, g = plms_case()
    model = get_model(False)
    mask = T(g["mask"]).to(DEV)
    noises = [g[f"noise_{i:03d}"] for i in range(len(g["draw_shapes"]))]
    with RecordRandnLike(replay=noises) as rec:
        out = run_masked(model, case, inp, mask, T(g["x0"]).to(DEV))
    assert rec.shapes == g["draw_shapes"].tolist()
    r = rel_l2(out, T(g["out"]))
    print(f"[plms_inpaint_tiny] rel_l2={r:.3e}")
    assert torch.isfinite(out).all() and r < 3.1e-3, r


# ------------------------------------------------------------------------------------------- interface end to end
@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt_inpaint")
    p = str(d / "tiny_gligen_inpaint.pth")
    ck = stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)
    ck["autoencoder"].update({k: torch.from_numpy(np.asarray(v)) for k, v in recipe.vae_encoder_state_dict(VAE_TINY, 0).items()})
    torch.save(ck, p)
    stubs.install_fake_sng_parser()
    am = itf.load_all_models(p, DEV)
    return p, am, stubs.toy_clip().to(DEV), stubs.ToyProcessor()


def _input_image():
    from PIL import Image
    a = (np.clip(recipe.uniform("inp.img", (40, 56, 3), 4), 0, 1) * 255).astype(np.uint8)
    return Image.fromarray(a)


def test_run_one_image_inpaints_like_the_manual_chain(loaded, tmp_path):
    p, am, clip, proc = loaded
    model, autoencoder, text_encoder, diffusion, config = am
    img = _input_image()
    loc = [[0.10, 0.10, 0.50, 0.55], [0.55, 0.20, 0.90, 0.70]]
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=loc, alpha_type=[0.5, 0.0, 0.5], input_image=img)
    args = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)
    seen = {}
    orig = itf.denoise

    def spy(*a, **k):
        seen["a"], seen["k"] = a, k
        return orig(*a, **k)
    itf.denoise = spy
    try:
        model.first_conv_type = "GLIGEN"
        torch.manual_seed(21)
        noise = torch.randn(2, 4, 16, 16).to(DEV)
        imgs = itf.run_one_image(am, args, meta, noise, clip, proc, device=DEV)
    finally:
        itf.denoise = orig
    # manual chain under the same seeds: encode -> mask -> sample(mask, x0) -> decode -> postprocess
    model.first_conv_type = "GLIGEN"
    torch.manual_seed(21)
    noise2 = torch.randn(2, 4, 16, 16).to(DEV)
    x = itf.load_input_image(img, 32, DEV)             # f * L = 2 * 16 for VAE_TINY
    assert x.shape == (1, 3, 32, 32) and float(x.min()) >= -1 and float(x.max()) <= 1
    z0 = autoencoder.encode(x)
    context, uc, relations, batch = seen["a"][1:5]
    mask = host.draw_masks_from_boxes(batch["boxes"], 16).to(DEV)
    assert torch.equal(seen["k"]["mask"], mask) and torch.equal(seen["k"]["x0"], z0) and z0.shape == (1, 4, 16, 16)
    lat = orig(am, context, uc, relations, batch, noise2, [0.5, 0.0, 0.5], 7.5, steps=4, mask=mask, x0=z0)
    ref = itf._postprocess(autoencoder.decode(lat))
    assert len(imgs) == 2 and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(imgs, ref))
    # the known region is kept: outside the boxes the final latent stays close to x0 (the last blend was at t = 1)
    keep = mask.bool().expand_as(lat)
    assert float((lat - z0.expand_as(lat))[keep].abs().mean()) < float((lat - z0.expand_as(lat))[~keep].abs().mean())


def test_run_batch_images_and_gligen_inference_with_input_images(loaded, tmp_path):
    p, am, clip, proc = loaded
    model = am[0]
    img = _input_image()
    path = str(tmp_path / "in.png")
    img.save(path)
    meta = dict(prompts=["cat sitting on mat", "a quiet street"], phrases=[["cat"], ["street"]],
                locations=[[[0.1, 0.1, 0.5, 0.5]], [[0.0, 0.5, 1.0, 1.0]]], alpha_type=[0.5, 0.0, 0.5], input_image=[img, path])
    model.first_conv_type = "GLIGEN"
    imgs = itf.run_batch_images(am, dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4), meta,
                                torch.randn(2, 4, 16, 16).to(DEV), clip, proc, device=DEV)
    assert len(imgs) == 2 and imgs[0].size == (32, 32)
    from layoutllm_t2i_amd import gligen_inference as gi
    gi._MODELS[p] = am
    m1 = dict(ckpt=p, prompt="cat sitting on mat", phrases=["cat"], locations=[[0.1, 0.1, 0.5, 0.5]], save_folder_name="inp",
              input_image=path)
    cfg = dict(batch_size=1, guidance_scale=7.5, no_plms=False, folder=str(tmp_path), device=DEV, steps=4)
    out = gi.run(m1, cfg, starting_noise=torch.randn(1, 4, 16, 16).to(DEV), clip_model=clip, clip_processor=proc)
    assert len(out) == 1 and os.path.exists(tmp_path / "inp" / "0.png")
