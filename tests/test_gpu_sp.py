"""The spatial grounding families (GLIGEN's canny / hed / depth / normal checkpoints) on the GPU: every kernel of csrc/spatial.hip against its
torch expression, the whole ConvNeXt tokenizer against tests/sp_ref.py and the reference's own outputs, TINY-width UNets with a grounding
downsampler through the engine against ``openaimodel_original`` goldens (tests/golden/sp_*.npz), batched CFG, and the interface on a synthetic
canny checkpoint."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import sp_cases as sc
import sp_ref
import stubs
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import ops, recipe, spatial
from layoutllm_t2i_amd._lib import HipLibraryError, init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.model import SpatialGroundingNetInput, UNetModel
from test_gpu_kernels import check
from test_gpu_model import rel_l2, report

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
NAN = float("nan")
KEYS = sp_ref.KEYS


def rnd(tag, shape, scale=1.0):
    return T(recipe.normal(f"gpusp.{tag}", tuple(shape), 47)) * scale


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


def _ord16(t):
    """fp16 values as integers that count representable values (adjacent values differ by 1; +0 and -0 coincide)"""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def assert_fp16_of(out16, ref64, name):
    """``out16`` is the fp32 result rounded to fp16: at most 1 fp16 ulp from the fp16 rounding of the fp64 reference"""
    out16 = out16.cpu()
    assert out16.dtype == torch.float16 and torch.isfinite(out16.float()).all(), name
    d = (_ord16(out16) - _ord16(ref64.to(torch.float16))).abs()
    print(f"[{name}] max fp16 ulps = {int(d.max())}, off by one: {float((d == 1).float().mean()):.2e}")
    assert int(d.max()) <= 1, (name, int(d.max()))


# ------------------------------------------------------------------------------------------- depthwise 7x7 + LayerNorm
DW_CASES = [(16, 16, 96), (8, 8, 192), (4, 4, 384), (2, 2, 768), (9, 5, 96)]


@pytest.mark.parametrize("H,W,C", DW_CASES, ids=[f"{h}x{w}-C{c}" for h, w, c in DW_CASES])
def test_dwconv_ln(H, W, C):
    """F.conv2d(groups=C, padding=3) + F.layer_norm(eps 1e-6) in fp32, the tolerance of test_gpu_kernels.py::test_layernorm_fp32_stream_and_stats
    (an fp16-output LayerNorm of fp32 rows); 4 x 4 and 2 x 2: every tap meets the zero border; 9 x 5: a partial pixel tile, two tiles per
    row at 16; pad columns [C, ld) exactly zero (the buffer starts as NaN), NaN sentinels around the output stay NaN"""
    B = 2
    x = rnd(f"dwx{H}.{W}.{C}", (B, H, W, C)) * 1.5 + 0.2
    w = rnd(f"dww{C}", (C, 1, 7, 7)) * (3.0 / 49) ** 0.5
    bias, gam, bet = 0.1 * rnd(f"dwb{C}", (C,)), 1 + 0.1 * rnd(f"dwg{C}", (C,)), 0.1 * rnd(f"dwe{C}", (C,))
    ld = (C + 63) // 64 * 64
    n, G = B * H * W * ld, 128
    buf = torch.full((2 * G + n,), NAN, dtype=torch.float16, device=DEV)
    out = buf[G:G + n].view(B * H * W, ld)
    d = lambda t: t.to(DEV).contiguous()
    ops.sp_dwconv_ln(d(x.reshape(B * H * W, C)), d(w.reshape(C, 49).t()), d(bias), d(gam), d(bet), B, H, W, out)
    conv = F.conv2d(x.permute(0, 3, 1, 2), w, bias, padding=3, groups=C).permute(0, 2, 3, 1)
    ref = F.layer_norm(conv, (C,), gam, bet, 1e-6).reshape(B * H * W, C)
    check(out[:, :C], ref, f"dwconv_ln {H}x{W} C{C}")
    h = buf.cpu()
    if ld > C:
        assert ld == 128 and float(h[G:G + n].view(-1, ld)[:, C:].float().abs().max()) == 0.0, "pad columns 96..127 must be written as zeros"
    assert torch.isnan(h[:G]).all() and torch.isnan(h[G + n:]).all(), "sentinel overwritten"


# ------------------------------------------------------------------------------------------- the small stages
def test_gelu():
    """0.5 x (1 + erf(x / sqrt 2)) in fp64 of the fp16 input, rounded to fp16: <= 1 ulp, the negative tail and the subnormals included"""
    x = torch.cat([rnd("gelu", (4096 - 66,)) * 2.0, torch.linspace(-8, 8, 64), torch.tensor([0.0, -0.0])]).half()
    y = ops.sp_gelu(x.to(DEV), torch.empty_like(x, device=DEV))
    x64 = x.double()
    assert_fp16_of(y, 0.5 * x64 * torch.special.erfc(-x64 * 0.5 ** 0.5), "gelu")
    z = x.to(DEV).clone()
    assert torch.equal(ops.sp_gelu(z, z), y), "in place"


@pytest.mark.parametrize("S,R", [(96, 64), (48, 64), (64, 64)], ids=["down", "up", "same"])
def test_stem_patchify(S, R):
    """F.interpolate (nearest) + unfold of 4x4 patches, K = (c, i, j), 48 -> 64 zero columns: exact (fp16 rounding of the selected value)"""
    B = 2
    m = rnd(f"map{S}", (B, 3, S, S))
    n, G = B * (R // 4) ** 2 * 64, 64
    buf = torch.full((2 * G + n,), NAN, dtype=torch.float16, device=DEV)
    out = ops.sp_stem_patchify(m.to(DEV), R, buf[G:G + n].view(-1, 64))
    r = F.interpolate(m, R)
    ref = F.unfold(r, 4, stride=4).transpose(1, 2).reshape(-1, 48)           # [B * L, (c, i, j)]
    h = buf.cpu()
    assert torch.equal(out.cpu()[:, :48], ref.half()) and float(out.cpu()[:, 48:].float().abs().max()) == 0.0
    assert torch.isnan(h[:G]).all() and torch.isnan(h[G + n:]).all(), "sentinel overwritten"


def test_layernorm_rows_and_down_gather():
    """the fp32 row LayerNorm (stem) and the per-pixel LayerNorm + 2x2 gather: fp16 rows exact up to 1 ulp of the fp64 expression"""
    B, H, W, C = 2, 6, 4, 96
    x = rnd("dgx", (B, H, W, C)) * 2 + 0.3
    gam, bet = 1 + 0.1 * rnd("dgg", (C,)), 0.1 * rnd("dgb", (C,))
    d = lambda t: t.to(DEV).contiguous()
    ref64 = F.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-6)
    y = ops.sp_layernorm(d(x.reshape(-1, C)), d(gam), d(bet), torch.empty(B * H * W, C, device=DEV))
    np.testing.assert_allclose(y.cpu().numpy(), ref64.reshape(-1, C).float().numpy(), rtol=1e-5, atol=2e-6)
    out = ops.sp_down_gather(d(x.reshape(-1, C)), d(gam), d(bet), B, H, W, torch.full((B * 3 * 2, 4 * C), NAN, dtype=torch.float16, device=DEV))
    ref = ref64.view(B, 3, 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * 3 * 2, 4 * C)      # (b, oy, ky, ox, kx, c) -> (b, oy, ox, ky, kx, c)
    assert_fp16_of(out, ref, "down_gather")
    # as the operand of the 2x2 stride-2 conv with the packed weight [Cout, (ky, kx, Cin)]
    w = rnd("dgw", (64, C, 2, 2)) * 0.05
    got = ops.gemm(out, d(w.permute(0, 2, 3, 1).reshape(64, 4 * C).half()), torch.empty(B * 6, 64, dtype=torch.float32, device=DEV))
    n16 = out.cpu().float().view(B, 3, 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)       # the same fp16 operands, as an image
    want = F.conv2d(n16.permute(0, 3, 1, 2), w.half().float(), stride=2).permute(0, 2, 3, 1).reshape(B * 6, 64)
    check(got, want, "down conv as gemm")


def test_token_assembly():
    """feat * m + null * (1 - m) + pos with masks 0 and 1 (and a fractional one) in one batch"""
    B, Tn, C = 3, 4, 768
    feat, null, pos = rnd("asf", (B * Tn, C)) * 2, rnd("asn", (C,)) * 0.5, rnd("asp", (Tn, C)) * 0.5
    m = torch.tensor([1.0, 0.0, 0.25])
    d = lambda t: t.to(DEV).contiguous()
    out = ops.sp_assemble(d(feat), d(m), d(null), d(pos), B, Tn, torch.empty(B * Tn, C, dtype=torch.float16, device=DEV))
    m64 = m.double().view(B, 1, 1)
    ref = feat.double().view(B, Tn, C) * m64 + null.double() * (1 - m64) + pos.double()
    assert_fp16_of(out, ref.view(B * Tn, C), "assemble")
    assert torch.equal(out.cpu().view(B, Tn, C)[1], (null + pos).half())       # the masked-out sample: null + pos, whatever the features


# ------------------------------------------------------------------------------------------- the downsampler's kernels
@pytest.mark.parametrize("n_in,n_out,C,Ct", [(128, 64, 1, 3), (128, 64, 3, 3), (512, 64, 1, 3), (96, 64, 1, 3), (64, 128, 3, 3)],
                         ids=["128-64-c1", "128-64-c3", "512-64-hed", "96-64", "64-128-up"])
def test_bicubic(n_in, n_out, C, Ct):
    """F.interpolate(mode="bicubic") of the first C channels, fp32: rtol 1e-5 / atol 1e-6 (sums of 16 fp32 products of O(1) values)"""
    B = 2
    x = T(recipe.uniform(f"gpusp.bic{n_in}", (B, Ct, n_in, n_in), 47))
    idx, w = spatial.bicubic_table(n_in, n_out)
    d = lambda a: T(a).to(DEV).contiguous()
    out = ops.sp_bicubic(x.to(DEV), C, d(idx), d(w), d(idx), d(w), torch.full((B, C, n_out, n_out), NAN, device=DEV))
    ref = F.interpolate(x[:, :C], (n_out, n_out), mode="bicubic")
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("Ci,Co,n,silu", [(1, 4, 64, True), (3, 4, 64, True), (4, 8, 32, False), (4, 8, 6, False)],
                         ids=["1-4-silu-64", "3-4-silu-64", "4-8-32", "4-8-6"])
def test_conv4x4s2(Ci, Co, n, silu):
    """Conv2d(Ci, Co, 4, 2, 1) (+ SiLU), fp32: rtol 1e-5 / atol 1e-6 (<= 64 fp32 products of O(1) values: 64 * 2^-24 = 4e-6 relative)"""
    B = 2
    x, w, b = rnd(f"cvx{Ci}.{n}", (B, Ci, n, n)), rnd(f"cvw{Ci}.{Co}", (Co, Ci, 4, 4)) * (3.0 / (16 * Ci)) ** 0.5, rnd(f"cvb{Co}", (Co,)) * 0.1
    out = ops.sp_conv4x4s2(x.to(DEV), w.to(DEV), b.to(DEV), silu, torch.full((B, Co, n // 2, n // 2), NAN, device=DEV))
    ref = F.conv2d(x, w, b, stride=2, padding=1)
    np.testing.assert_allclose(out.cpu().numpy(), (F.silu(ref) if silu else ref).numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", sc.DS_CASES, ids=[c["name"] for c in sc.DS_CASES])
def test_downsampler_matches_reference_golden(case):
    """SpatialDownsampler (128 -> 64 -> 32 -> 16; hed 512 -> 64) against the reference's own output, the fp32 tolerance of its kernels"""
    cfg = sc.cfg_of(case)
    sd = recipe.state_dict(cfg, 0, only_prefix="downsample_net.")
    ds = spatial.SpatialDownsampler({k: T(np.asarray(v)) for k, v in sd.items()}, cfg, DEV)
    out = ds(T(sc.case_inputs(case)["map"]))
    ref = np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"]
    assert tuple(out.shape) == ref.shape == (case["B"], cfg.ds_out, cfg.ds_latent, cfg.ds_latent)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------- the whole tokenizer
@pytest.mark.parametrize("case", sc.POSNET_CASES, ids=[c["name"] for c in sc.POSNET_CASES])
def test_tokenizer_matches_sp_ref_and_the_reference(case):
    """T = 4 (resize 64) and T = 64 (resize 256), B = 2, sample 1 masked out.  The bound is MEASURED: tests/sp_ref.py with every matrix operand
    rounded to fp16 (fp32 accumulate) against fp32 sp_ref gives the cost of the stage's arithmetic; the GPU result has to be within 2 x that
    of fp32 sp_ref and of the reference's own output (the summation order is the only other difference).  The masked-out sample's tokens are
    the cached null tokens bit for bit."""
    cfg = sc.cfg_of(case)
    sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(cfg, 0, only_prefix="position_net.").items()}
    inp = {a: T(v) for a, v in sc.case_inputs(case).items()}
    with torch.no_grad():
        ref32 = sp_ref.position_net(sd, cfg, inp["map"], inp["mask"])
        ref16 = sp_ref.position_net(sd, cfg, inp["map"], inp["mask"], q=sp_ref.fp16_operands)
    gold = T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out_canny"])
    tok = spatial.SpatialTokenizer(sd, cfg, DEV)
    out = tok.tokens(inp["map"], inp["mask"])
    assert tuple(out.shape) == tuple(gold.shape) == (2, cfg.n_ground, cfg.pos_out_dim) and out.dtype == torch.float32
    bound = rel_l2(ref16, ref32)
    r, rg, re = rel_l2(out, ref32), rel_l2(out, gold), rel_l2(out, ref16)
    print(f"[{case['name']}] fp16-operand sp_ref vs fp32 sp_ref rel_l2 = {bound:.3e}; GPU vs fp32 sp_ref {r:.3e}, vs golden {rg:.3e}, "
          f"vs fp16-operand sp_ref {re:.3e}")
    assert torch.isfinite(out).all() and 1e-5 < bound < 1e-2
    assert r < 2 * bound and rg < 2 * bound, (r, rg, bound)
    null = tok.null_tokens()
    assert torch.equal(out[1], null[0]), "masked-out sample == cached null tokens"
    assert tok.null_tokens() is null                                           # computed once
    assert rel_l2(out[0], null[0]) > 1e-2                                      # the other sample sees its map
    allnull = tok.tokens(inp["map"], torch.zeros(2))
    assert torch.equal(allnull[0], null[0]) and torch.equal(allnull[1], null[0])
    with pytest.raises(ValueError, match="mask has 3"):
        tok.tokens(inp["map"], torch.ones(3))


# ------------------------------------------------------------------------------------------- whole model: tiny UNets vs the reference
_models = {}


def get_model(family):
    if family not in _models:
        cfg = sc.HED_TINY if family == "hed" else sc.CANNY_TINY
        m = UNetModel(cfg, recipe.state_dict(cfg, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(cfg, 0))
        m.grounding_tokenizer_input = SpatialGroundingNetInput()
        _models[family] = m
    return _models[family]


def _load(case):
    return {a: T(v) for a, v in sc.case_inputs(case).items()}, T(np.load(os.path.join(GOLD, case["name"] + ".npz"))["out"])


def _golden_call(model, case, inp, extra=None):
    model.fuser_scale = case["scale"]
    model.first_conv_type = "SD" if case["sdconv"] else "GLIGEN"
    g = model.grounding_tokenizer_input.prepare({k: inp[k] for k in KEYS})
    ctx = inp["context"]
    if case["grounding"] == "null":
        g, ctx = model.grounding_tokenizer_input.get_null_input(), inp["uc"]
    try:
        return model(dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=ctx, inpainting_extra_input=None,
                          grounding_extra_input=inp["map"] if extra is None else extra, grounding_input=g))
    finally:
        model.first_conv_type = "GLIGEN"


@pytest.mark.parametrize("case", sc.UNET_CASES, ids=[c["name"] for c in sc.UNET_CASES])
def test_tiny_unet_matches_reference_golden(case):
    """canny (12-channel conv, 16 x 16 latent, B = 2) and hed (5-channel, 64 x 64, B = 1) against openaimodel_original's output, default mode,
    the bound of tests/test_gpu_kp.py::test_tiny_unet_matches_reference_golden; graph replay == eager bitwise.  On the SD conv (fuser scale 0)
    the output does not depend on the extra: another map gives the same bits."""
    model = get_model(case["family"])
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
    other = _golden_call(model, case, inp, extra=-inp["map"].flip(-1))
    if case["sdconv"]:
        assert torch.equal(other, out), "the SD conv reads the latent alone"
    else:
        assert rel_l2(other, out) > 1e-3, "the GLIGEN conv reads the downsampled map"


def test_cfg_batched_2b_equals_two_calls():
    """[cond ; null] as one 2B batch == two B-sized calls within 1e-6 (tests/test_gpu_kp.py::test_cfg_batched_2b_equals_two_calls); both halves
    read the same extra"""
    model = get_model("canny")
    eng, tok = model.engine, model.tokenizer
    inp, _ = _load(sc.by_name("sp_unet_canny_s1"))
    x = inp["x"].to(DEV)
    objs, null = tok.tokens(inp["map"], inp["mask"]), tok.null_tokens().expand(2, -1, -1)
    extra = model.downsampler(inp["map"])
    assert tuple(extra.shape) == (2, 8, 16, 16)

    def one(ctx, o, reps):
        eng.set_conditioning_tokens(ctx, o, 16)
        eng.set_grounding_extra(extra)
        return eng.forward(x, 981.0, 1.0, False, reps).clone()
    ec, eu = one(inp["context"], objs, 1), one(inp["uc"], null, 1)
    e2 = one(torch.cat([inp["context"], inp["uc"]], 0), torch.cat([objs, null], 0), 2)
    rc, ru = rel_l2(e2[:2], ec), rel_l2(e2[2:], eu)
    print(f"[sp 2B] rel_l2 cond {rc:.2e} uncond {ru:.2e}")
    assert rc < 1e-6 and ru < 1e-6, (rc, ru)
    assert rel_l2(ec, eu) > 1e-2                        # the two halves are different problems


def test_engine_refusals():
    from layoutllm_t2i_amd import _lib
    model = get_model("canny")
    eng = model.engine
    inp, _ = _load(sc.by_name("sp_unet_canny_s1"))
    with pytest.raises(ValueError, match="boxes given to a spatial model"):
        eng.set_conditioning(inp["context"], None, torch.zeros(2, 4, 4), torch.zeros(2, 4), torch.zeros(2, 4, 768), 16)
    with pytest.raises(ValueError, match=r"\[Bn, 4, 768\]"):
        eng.set_conditioning_tokens(inp["context"], torch.zeros(2, 5, 768), 16)
    objs = model.tokenizer.null_tokens().expand(2, -1, -1)
    eng.set_conditioning_tokens(inp["context"], objs, 32)                      # a new latent shape: the extra has to be set again
    with pytest.raises(HipLibraryError, match="gl_set_grounding_extra"):
        eng.forward(torch.zeros(2, 4, 32, 32, device=DEV), 981.0, 1.0, False, 1)
    with pytest.raises(ValueError, match=r"need \[1 \| samples, 8, 32, 32\]"):
        eng.set_grounding_extra(torch.zeros(2, 8, 16, 16))
    eng.forward(torch.zeros(2, 4, 32, 32, device=DEV), 981.0, 0.0, True, 1)    # the SD conv needs no extra
    text = UNetModel(dataclasses.replace(TINY, relation=False), recipe.state_dict(dataclasses.replace(TINY, relation=False), 0), device=DEV)
    with pytest.raises(ValueError, match="spatial grounding needs"):
        text.engine.set_conditioning_tokens(inp["context"], objs, 16)
    with pytest.raises(ValueError, match="without a grounding downsampler"):
        text.engine.set_grounding_extra(torch.zeros(2, 8, 16, 16))
    with pytest.raises(ValueError, match="grounding_extra_input"):
        model(dict(x=inp["x"].to(DEV), timesteps=torch.tensor([981, 981]), context=inp["context"], grounding_input={k: inp[k] for k in KEYS}))


# ------------------------------------------------------------------------------------------- the interface
def _write_canny_checkpoint(path):
    """stubs.write_synthetic_checkpoint's container with the model of a canny checkpoint: the tokenizer / downsampler targets and tensors, no
    ``*.rela_fuse.*`` tensor"""
    ck = stubs.write_synthetic_checkpoint(path, TINY, VAE_TINY, max_relations=10)
    cfg = sc.CANNY_TINY
    tok, ds = sc.targets("canny")
    params = ck["config_dict"]["_content"]["model"]["params"]
    params["grounding_tokenizer"] = {"target": tok, "params": {"resize_input": cfg.sp_resize_input, "out_dim": 768}}
    params["grounding_downsampler"] = {"target": ds, "params": {"resize_input": cfg.ds_resize_input, "out_dim": 8}}
    ck["config_dict"]["_content"]["grounding_tokenizer_input"]["target"] = "grounding_input.canny_grounding_tokinzer_input.GroundingNetInput"
    ck["model"] = {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in recipe.state_dict(cfg, 0).items()}
    torch.save(ck, path)
    return ck


def test_interface_on_a_canny_checkpoint(tmp_path):
    """load_all_models, run_one_image, run_batch_images and gligen_inference.run with 4 steps and alpha_type [0.5, 0, 0.5] (both first convs
    run), no phrases and no CLIP model: image sizes, the same seed gives the same image on the cached model, and the refusals"""
    from PIL import Image
    p = str(tmp_path / "tiny_gligen_canny.pth")
    ck = _write_canny_checkpoint(p)           # (the small backbone: load_ckpt reads depths and widths off the checkpoint's tensors)
    with pytest.raises(NotImplementedError, match="strict"):
        itf.load_all_models(p, DEV, strict=True)
    am = itf.load_all_models(p, DEV)
    model, autoencoder = am[0], am[1]
    assert isinstance(model.grounding_tokenizer_input, SpatialGroundingNetInput) and model.cfg == dataclasses.replace(sc.CANNY_TINY)
    assert model.first_conv_restorable and model.tokenizer is not None and model.downsampler.out_side == 16
    img = str(tmp_path / "edges.png")
    Image.fromarray(sc.test_image()).save(img)
    prompt, alpha_type, S = "a house by a lake", [0.5, 0.0, 0.5], 4
    args = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=S)
    meta = dict(prompt=prompt, canny_image=img, alpha_type=alpha_type)
    torch.manual_seed(123)
    noise = torch.randn(2, 4, 16, 16)
    dec = autoencoder.decode

    def run(meta_=meta, args_=args):
        captured = {}
        autoencoder.decode = lambda lat: dec(captured.setdefault("lat", lat.clone()))
        model.first_conv_type = "GLIGEN"
        try:
            imgs = itf.run_one_image(am, dict(args_), meta_, noise.to(DEV), None, None, device=DEV)
        finally:
            autoencoder.decode = dec
        assert len(imgs) == 2 and imgs[0].size == (32, 32) and imgs[0].mode == "RGB"
        assert model.first_conv_type == "SD", "the scale-0 steps switched to the SD conv"
        return captured["lat"], imgs
    lat, imgs = run()
    assert torch.isfinite(lat).all()
    lat2, imgs2 = run()
    assert torch.equal(lat2, lat) and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(imgs, imgs2)), "a second run, cached model"
    flipped = str(tmp_path / "flipped.png")
    Image.open(img).transpose(Image.FLIP_LEFT_RIGHT).save(flipped)
    assert rel_l2(run(dict(meta, canny_image=flipped))[0], lat) > 1e-3, "the map enters"
    assert rel_l2(run(args_=dict(args, negative_prompt="blurry"))[0], lat) > 1e-3, "negative_prompt enters"
    model.first_conv_type = "GLIGEN"
    both = itf.run_batch_images(am, dict(args), dict(prompts=[prompt, "a barn"], canny_image=[img, Image.open(flipped)], alpha_type=alpha_type),
                                noise.to(DEV), None, None, device=DEV)
    assert len(both) == 2 and both[0].size == (32, 32)
    from layoutllm_t2i_amd import gligen_inference as gi
    gi._MODELS[p] = am
    try:
        out = gi.run(dict(ckpt=p, prompt=prompt, canny_image=img, alpha_type=alpha_type),
                     dict(batch_size=1, guidance_scale=7.5, no_plms=False, device=DEV, steps=S), starting_noise=torch.randn(1, 4, 16, 16).to(DEV))
        assert len(out) == 1 and out[0].size == (32, 32)
        with pytest.raises(NotImplementedError):
            gi.run(dict(ckpt=p, prompt=prompt, canny_image=img), dict(batch_size=1, guidance_scale=7.5, no_plms=True, device=DEV, steps=S),
                   starting_noise=torch.randn(1, 4, 16, 16).to(DEV))
    finally:
        gi._MODELS.pop(p, None)
    # refusals, before any kernel runs
    n = noise.to(DEV)
    with pytest.raises(ValueError, match=r"meta\['input_image'\]"):
        itf.run_one_image(am, dict(args), dict(meta, input_image=img), n, None, None, device=DEV)
    with pytest.raises(ValueError, match=r"meta\['images'\]"):
        itf.run_one_image(am, dict(args), dict(meta, images=[img]), n, None, None, device=DEV)
    with pytest.raises(ValueError, match=r"meta\['locations'\]"):
        itf.run_one_image(am, dict(args), dict(meta, locations=[[0.1, 0.1, 0.4, 0.4]], phrases=["a house"]), n, None, None, device=DEV)
    with pytest.raises(ValueError, match="16 x 16"):
        itf.run_one_image(am, dict(args), meta, torch.randn(2, 4, 16, 24).to(DEV), None, None, device=DEV)
    with pytest.raises(ValueError, match="needs its map"):
        itf.run_one_image(am, dict(args), dict(prompt=prompt, alpha_type=alpha_type), n, None, None, device=DEV)
    # the sampler itself: a missing grounding_extra_input is refused before any kernel runs
    from layoutllm_t2i_amd.model import LatentDiffusion
    from layoutllm_t2i_amd.sampler import PLMSSampler
    batch = itf.prepare_batch_spatial(meta, 2, DEV)
    g = model.grounding_tokenizer_input.prepare(batch)
    ctx = torch.zeros(2, 77, 768)
    with pytest.raises(ValueError, match="grounding_extra_input"):
        PLMSSampler(LatentDiffusion(device=DEV), model).sample(S=2, shape=(2, 4, 16, 16),
                                                                input=dict(x=n, timesteps=None, context=ctx, grounding_input=g), uc=ctx, guidance_scale=7.5)
    # a checkpoint that lacks a tokenizer tensor names it
    bad = dict(ck, model={k: v for k, v in ck["model"].items() if k != "position_net.pos_embedding"})
    pb = str(tmp_path / "bad.pth")
    torch.save(bad, pb)
    with pytest.raises(KeyError, match="pos_embedding"):
        itf.load_all_models(pb, DEV)
