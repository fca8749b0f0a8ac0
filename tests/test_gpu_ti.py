"""The text_image grounding family (GLIGEN's *_box_text_image checkpoints) on the GPU: the two new kernels, the fuser's attention at the
new key counts N + 60 in the engine's layout, the tiny UNet against the reference's own outputs (tests/golden/ti_*.npz) in default and
strict mode, one full-width level against tests/ti_ref.py, and the interface boundary with reference images."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import stubs
import ti_cases as tc
import ti_ref
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import ops, recipe
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, UNetConfig
from layoutllm_t2i_amd.model import TextImageGroundingNetInput, UNetModel
from layoutllm_t2i_amd.weights import q_fold
from oracle import plms_ref, unet_ref, vae_ref
from test_gpu_attention_layouts import _attn_exp2, expect_form
from test_gpu_kernels import _attn_ref, check
from test_gpu_model import _fp16_representable, oracle_sd, rel_l2, report
from test_gpu_strict import rel, split

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
NAN = float("nan")
SENT = -999.0
KEYS = ti_ref.KEYS


def rnd(tag, shape, scale=1.0):
    return T(recipe.normal(f"gputi.{tag}", tuple(shape), 41)) * scale


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


# ------------------------------------------------------------------------------------------- posnet_input_ti
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_posnet_input_ti(dtype):
    """both MLP inputs in one launch vs the torch expression of text_image_grounding_net.py:48-61; the tolerances of
    test_gpu_kernels.py::test_posnet_input_and_timestep_embedding; NaN sentinels before, between and behind the two outputs stay NaN"""
    B, mo, dim = 2, 30, 768
    boxes = T(np.abs(recipe.uniform("gputi.pb", (B, mo, 4), 3)))
    masks, tm, im = torch.zeros(B, mo), torch.zeros(B, mo), torch.zeros(B, mo)
    masks[0, :5] = 1
    masks[1, :2] = 1
    tm[0, [0, 2, 3]] = 1
    im[0, [1, 2, 4]] = 1
    tm[1, 0] = 0.5                                       # meta["text_mask"] may scale a mask: a true blend, not a select
    im[1, 1] = 1
    te, ie = rnd("te", (B, mo, dim)), rnd("ie", (B, mo, dim))          # non-zero on every row: a mask that is ignored shows
    nt, ni, nxy = rnd("nt", (dim,), 0.5), rnd("ni", (dim,), 0.5), rnd("nx", (64,), 0.5)
    n, G = B * mo * (dim + 64), 128
    buf = torch.full((3 * G + 2 * n,), NAN, dtype=dtype, device=DEV)
    ot, oi = buf[G:G + n].view(B * mo, dim + 64), buf[2 * G + n:2 * G + 2 * n].view(B * mo, dim + 64)
    d = lambda x: x.to(DEV)
    ops.posnet_input_ti(d(boxes), d(masks), d(tm), d(im), d(te), d(ie), d(nt), d(ni), d(nxy), 8, ot, oi)
    m_, tm_, im_ = masks.unsqueeze(-1), tm.unsqueeze(-1), im.unsqueeze(-1)
    xy = unet_ref.fourier_embed(boxes, 8) * m_ + (1 - m_) * nxy
    check(ot, torch.cat([te * tm_ + (1 - tm_) * nt, xy], -1).view(B * mo, -1), f"posnet_input_ti text {dtype}")
    check(oi, torch.cat([ie * im_ + (1 - im_) * ni, xy], -1).view(B * mo, -1), f"posnet_input_ti image {dtype}")
    assert torch.equal(ot[:, dim:], oi[:, dim:]), "the Fourier part is computed once"
    h = buf.cpu()
    for a, b in ((0, G), (G + n, 2 * G + n), (2 * G + 2 * n, 3 * G + 2 * n)):
        assert torch.isnan(h[a:b]).all(), "sentinel overwritten"


# ------------------------------------------------------------------------------------------- gl_image_ground_feature
@pytest.mark.parametrize("n,dim", [(1, 64), (5, 64), (1, 768), (5, 768)])
def test_image_ground_feature(n, dim):
    """28.7 * (f P) / ||f P|| vs fp64.  Bound: 4 x the distance that torch's own fp32 evaluation of the same expression has to fp64 on these
    inputs (L2 over the whole output); the norm of every output row equals 28.7 to fp32 rounding of a sqrt of a sum of dim squares."""
    f, P = rnd(f"f{n}.{dim}", (n, dim)), rnd(f"P{dim}", (dim, dim), dim ** -0.5)
    G = 64
    buf = torch.full((2 * G + n * dim,), NAN, dtype=torch.float32, device=DEV)
    out = buf[G:G + n * dim].view(n, dim)
    ops.image_ground_feature(f.to(DEV), P.to(DEV), 28.7, out)
    y64 = f.double() @ P.double()
    want = y64 / y64.norm(dim=-1, keepdim=True) * 28.7
    y32 = f @ P
    t32 = y32 / y32.norm(dim=-1, keepdim=True) * 28.7
    e_torch = float((t32.double() - want).norm())
    e = float((out.cpu().double() - want).norm())
    print(f"[image_ground_feature n={n} dim={dim}] |err|_2 = {e:.3e}, torch fp32 {e_torch:.3e}, bound {4 * e_torch:.3e}")
    assert torch.isfinite(out).all() and e <= 4 * e_torch, (e, e_torch)
    norms = out.cpu().double().norm(dim=-1)
    # fp32 rounding of that norm, u = 2^-24: the sum of squares is a tree of at most 12 additions over rounded squares (3 in a thread, 6 across
    # the wave, 3 across the waves): 13 u relative, halved by the square root; + u/2 each for the square root, the division, the product and
    # for 28.7 itself as an fp32 number: 8.5 u on the norm, asserted as 10 u
    assert float((norms - 28.7).abs().max()) <= 10 * 28.7 * 2.0 ** -24, norms
    h = buf.cpu()
    assert torch.isnan(h[:G]).all() and torch.isnan(h[G + n * dim:]).all(), "sentinel overwritten"


# ------------------------------------------------------------------------------------------- fuser attention at N + 60 keys
# (d, N): Nk = N + 60 = 64 (exactly one key tile; the text path's smallest Nk is 34), 124, 316, 1084
FUSER_CASES = [(16, 4, "f16_4w_pre0", "split_4w_dbuf"), (16, 256, "f16_4w_pre0", "split_4w_dbuf"), (40, 64, "f16_4w_pre2", "split_4w_dbuf"),
               (40, 256, "f16_4w_pre2", "split_4w_dbuf"), (80, 1024, "f16_8w_pre1", "split_4w_dbuf"), (160, 64, "f16_4w_pre1", "split_4w_single")]


def _engine_layout_launch(qh, ql, kh, kl, vh, vl, B, H, d, N, Nk, rows, split_ops):
    """gl_attention as engine.hip's self_attention launches the fuser: ONE [B * rows, 3 S C] buffer of [q k v (| q_lo k_lo v_lo)] rows,
    rows = N + 64 per sample, Nq = N = rows - 64 queries, Nk = N + 60 keys; the 4 pad rows (and the q columns of the token rows, which are
    never queries) are NaN; V^T hi / lo are the halves of one allocation with row stride vt_ld(rows), NaN behind key Nk; the output is
    [B * N, S C] with sentinel rows behind it."""
    C, S = H * d, 2 if split_ops else 1
    pad = lambda x, fill: torch.cat([x, torch.full((B, rows - x.shape[1], C), fill, dtype=torch.float16)], 1)
    hi3 = torch.cat([pad(qh, NAN), pad(kh, NAN), pad(vh, NAN)], 2)
    full = torch.cat([hi3, torch.cat([pad(ql, NAN), pad(kl, NAN), pad(vl, NAN)], 2)], 2) if split_ops else hi3
    buf = full.reshape(B * rows, 3 * S * C).contiguous().to(DEV)
    ld6, bs = 3 * S * C, rows * 3 * S * C
    ld = ops.vt_ld(rows)
    vt2 = torch.full((S, B, H, d, ld), NAN, dtype=torch.float16, device=DEV)
    for s in range(S):
        ops.transpose_v(buf[:, s * 3 * C + 2 * C:], bs, ld6, vt2[s], B, H, d, Nk)
    vt2[..., Nk:] = NAN
    out = torch.full((B * N + 264, S * C), SENT, dtype=torch.float16, device=DEV)
    kw = dict(q_lo=buf[:, 3 * C:], k_lo=buf[:, 4 * C:], vt_lo=vt2[1], out_lo=out[:, C:]) if split_ops else {}
    ops.attention(buf, bs, ld6, buf[:, C:], bs, ld6, vt2[0], out, N * S * C, S * C, B, H, d, N, Nk, 123.0, q_prescaled=True, **kw)
    o = out.cpu()
    assert torch.isfinite(o[:B * N]).all(), "non-finite output: a NaN pad row / pad key was consumed"
    assert bool((o[B * N:] == SENT).all()), "rows behind the output overwritten"
    return o[:B * N].view(B, N, S * C)


@pytest.mark.parametrize("d,N,f16_form,split_form", FUSER_CASES, ids=[f"d{c[0]}-N{c[1]}" for c in FUSER_CASES])
def test_fuser_attention_at_text_image_key_counts(d, N, f16_form, split_form):
    """single-fp16 and split-fp16 kernels with the tolerances of test_gpu_kernels.py::test_attention_prescaled_q (rtol 2e-3 / atol 2e-4 vs
    fp32 on the same fp16 operands) and test_gpu_strict.py::test_split_attention (rel-L2 < 1e-6 vs fp64 of hi + lo, the single-fp16
    kernel > 20 x worse); each launch is attributed to the kernel form the dispatcher documents, by its launch counter"""
    B, H = 2, 2
    C, Nk, rows = H * d, N + 60, N + 64
    q, k, v = rnd(f"q{d}.{N}", (B, N, C)) * 1.2, rnd(f"k{d}.{N}", (B, Nk, C)) * 1.2, rnd(f"v{d}.{N}", (B, Nk, C))
    k[:, N + 45] = 3.0 * q[:, 1]                         # a dominant key among the image tokens (the last key tile)
    (qh, ql), (kh, kl), (vh, vl) = split(q * q_fold(d)), split(k), split(v)
    with expect_form(f16_form):
        o1 = _engine_layout_launch(qh, None, kh, None, vh, None, B, H, d, N, Nk, rows, False)
    check(o1, _attn_ref(qh.float() / q_fold(d), kh.float(), vh.float(), H), f"fuser attn f16 d{d} N{N} Nk{Nk}", rtol=2e-3, atol=2e-4)
    with expect_form(split_form):
        o2 = _engine_layout_launch(qh, ql, kh, kl, vh, vl, B, H, d, N, Nk, rows, True)
    f64 = lambda hi, lo: hi.double() + lo.double()
    want = _attn_exp2(f64(qh, ql), f64(kh, kl), f64(vh, vl), H)
    r, r1 = rel(o2[..., :C].double() + o2[..., C:].double(), want), rel(o1, want)
    print(f"[fuser attn split d={d} N={N} Nk={Nk}] rel_l2 = {r:.2e} (single-fp16 kernel {r1:.2e})")
    assert r < 1e-6 and r1 > 20 * r, (r, r1)


# ------------------------------------------------------------------------------------------- whole model: tiny UNet vs the reference
_models = {}


def get_model(split_weights=False):
    if split_weights not in _models:
        cfg = dataclasses.replace(tc.TI_TINY, split_weights=split_weights)
        m = UNetModel(cfg, recipe.state_dict(tc.TI_TINY, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(tc.TI_TINY, 0))
        m.grounding_tokenizer_input = TextImageGroundingNetInput()
        _models[split_weights] = m
    return _models[split_weights]


def _golden_call(model, case, inp, **override):
    model.fuser_scale = case["scale"]
    model.first_conv_type = "SD" if case["sdconv"] else "GLIGEN"
    g = model.grounding_tokenizer_input.prepare({**{k: inp[k] for k in KEYS}, **override})
    return model(dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], relations=inp["relations"],
                      inpainting_extra_input=None, grounding_extra_input=None, grounding_input=g))


UNET_CASES = [c for c in tc.CASES if c["kind"] == "unet"]


@pytest.mark.parametrize("case", UNET_CASES, ids=[c["name"] for c in UNET_CASES])
def test_tiny_unet_matches_reference_golden(case):
    """default mode, the bound of test_gpu_model.py::test_tiny_unet_matches_reference_golden; graph replay == eager bitwise; with the image
    masks zeroed the output moves by far more than the bound, so it cannot be met with the image tokens ignored (fuser on)"""
    model = get_model()
    inp = {a: T(v) for a, v in tc.case_inputs(case).items()}
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
    if case["scale"] != 0:
        moved = rel_l2(_golden_call(model, case, inp, image_masks=torch.zeros_like(inp["image_masks"])), ref)
        print(f"[{case['name']}] image masks zeroed: rel_l2 = {moved:.3e}")
        assert moved > 1e-3, moved


@pytest.mark.parametrize("case", UNET_CASES, ids=[c["name"] for c in UNET_CASES])
def test_tiny_unet_strict_matches_reference_golden(case):
    """strict mode on a split_weights handle, the bound of test_gpu_strict.py::test_tiny_unet_strict_vs_oracle_and_default"""
    model = get_model(True)
    inp = {a: T(v) for a, v in tc.case_inputs(case).items()}
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


def _set_cond(eng, inp, ctx_key, null, hw=16, idx=slice(None)):
    z = (lambda t: torch.zeros_like(t)) if null else (lambda t: t)
    eng.set_conditioning(inp[ctx_key][idx], inp["relations"][idx], z(inp["boxes"][idx]), z(inp["masks"][idx]), z(inp["text_embeddings"][idx]), hw,
                         text_masks=z(inp["text_masks"][idx]), image_masks=z(inp["image_masks"][idx]), image_embeddings=z(inp["image_embeddings"][idx]))


def test_cfg_batched_2b_equals_two_calls():
    """[cond ; uncond] as one 2B batch == two B-sized calls, as test_gpu_model.py::test_cfg_batched_2b_equals_two_calls asserts; the uncond
    half is all six grounding tensors zero"""
    eng = get_model().engine
    inp = {a: T(v) for a, v in tc.unet_inputs(tc.by_name("ti_unet_tiny_s1")).items()}
    x = inp["x"].to(DEV)
    _set_cond(eng, inp, "context", False)
    ec = eng.forward(x, 981.0, 1.0, False, 1).clone()
    _set_cond(eng, inp, "uc", True)
    eu = eng.forward(x, 981.0, 1.0, False, 1).clone()
    cat = lambda a, b: torch.cat([a, b], 0)
    z = torch.zeros_like
    eng.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
                         cat(inp["masks"], z(inp["masks"])), cat(inp["text_embeddings"], z(inp["text_embeddings"])), 16,
                         text_masks=cat(inp["text_masks"], z(inp["text_masks"])), image_masks=cat(inp["image_masks"], z(inp["image_masks"])),
                         image_embeddings=cat(inp["image_embeddings"], z(inp["image_embeddings"])))
    e2 = eng.forward(x, 981.0, 1.0, False, 2).clone()
    assert rel_l2(e2[:2], ec) < 1e-6 and rel_l2(e2[2:], eu) < 1e-6
    assert rel_l2(ec, eu) > 1e-2                        # the two halves are different problems


def test_lazy_strict_hoists_use_all_six_inputs():
    """a split handle conditioned in DEFAULT mode keeps device copies of its inputs (the four text_image ones included) and computes the
    strict hoists with the first strict forward: same bits as conditioning in strict mode; changing only the image inputs in between changes them"""
    model = get_model(True)
    eng = model.engine
    inp = {a: T(v) for a, v in tc.unet_inputs(tc.by_name("ti_unet_tiny_s1")).items()}
    x = inp["x"].to(DEV)
    model.set_strict(False)
    _set_cond(eng, inp, "context", False)
    eng.forward(x, 481.0, 1.0, False, 1)
    try:
        eng.set_option(50, 1)
        lazy = eng.forward(x, 481.0, 1.0, False, 1).clone()
        _set_cond(eng, inp, "context", False)
        direct = eng.forward(x, 481.0, 1.0, False, 1).clone()
        assert torch.equal(lazy, direct), "lazy hoists == hoists at conditioning time"
        eng.set_option(50, 0)
        inp2 = dict(inp, image_embeddings=inp["image_embeddings"] * 0.5, image_masks=inp["image_masks"] * 0.75, text_masks=inp["text_masks"] * 0.5)
        _set_cond(eng, inp2, "context", False)
        eng.set_option(50, 1)
        lazy2 = eng.forward(x, 481.0, 1.0, False, 1).clone()
        _set_cond(eng, inp2, "context", False)
        assert torch.equal(eng.forward(x, 481.0, 1.0, False, 1), lazy2)
        assert rel_l2(lazy2, lazy) > 1e-3
    finally:
        eng.set_option(50, 0)


def test_engine_refuses_the_other_family():
    from layoutllm_t2i_amd._lib import HipLibraryError
    eng = get_model().engine
    inp = {a: T(v) for a, v in tc.unet_inputs(tc.by_name("ti_unet_tiny_s1")).items()}
    with pytest.raises(ValueError, match="text_image model needs"):
        eng.set_conditioning(inp["context"], inp["relations"], inp["boxes"], inp["masks"], inp["text_embeddings"], 16)
    d = lambda t: t.to(DEV).contiguous()
    keep = [d(inp[k]) for k in ("context", "relations", "boxes", "masks", "text_embeddings")]
    rc = eng._lib.gl_set_conditioning(eng.handle, *(t.data_ptr() for t in keep), 2, 77, 10, 16, None)
    from layoutllm_t2i_amd import _lib
    assert rc == -1 and "grounding = 1 (text_image)" in _lib.last_error(eng.handle)


# ------------------------------------------------------------------------------------------- one full-width level
def test_default_mode_full_width_level_vs_ti_ref():
    """model_channels 320 (d = 40), one level, 16 x 16 (Nk = 316), [cond ; uncond] with one latent (2B = 2), against tests/ti_ref.py with
    fp16-representable weights; the bound of the text twin, test_default_mode_full_width_level_fp16_operand_bound_vs_oracle"""
    cfg = UNetConfig(image_size=16, model_channels=320, channel_mult=(1,), attention_resolutions=(1,), num_res_blocks=1, grounding="text_image")
    sd = _fp16_representable(recipe.state_dict(cfg, 0))
    model = UNetModel(cfg, sd, device=DEV)
    inp = {k: T(v) for k, v in recipe.synth_inputs(cfg, 1, 16, n_boxes=8, n_rel=3, seed=4321).items()}
    h16 = lambda t: t.half().float()
    g = {k: inp[k] for k in KEYS}
    gn = ti_ref.null_grounding(g)
    cat = lambda a, b: torch.cat([a, b], 0)
    model.engine.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(g["boxes"], gn["boxes"]),
                                  cat(g["masks"], gn["masks"]), cat(g["text_embeddings"], gn["text_embeddings"]), 16,
                                  text_masks=cat(g["text_masks"], gn["text_masks"]), image_masks=cat(g["image_masks"], gn["image_masks"]),
                                  image_embeddings=cat(g["image_embeddings"], gn["image_embeddings"]))
    out = model.engine.forward(h16(inp["x"]).to(DEV), 481.0, 1.0, False, 2).clone()
    t = torch.full((1,), 481, dtype=torch.long)
    osd = oracle_sd(sd)
    with torch.no_grad():
        torch.set_num_threads(min(32, max(1, os.cpu_count() or 1)))
        rc = ti_ref.unet_forward(osd, cfg, h16(inp["x"]), t, h16(inp["context"]), h16(inp["relations"]), g)
        ru = ti_ref.unet_forward(osd, cfg, h16(inp["x"]), t, h16(inp["uc"]), h16(inp["relations"]), gn)
    r = report("ti L0_c320_d40_16x16", out, cat(rc, ru))
    assert r < 7.5e-4, r
    del model
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- the boundary
class _Processor(stubs.ToyProcessor):
    """ToyProcessor for phrases; for ``images=[PIL.Image]`` the 224 x 224 pixel tensor of the toy CLIP's vision tower"""

    def __call__(self, text=None, return_tensors="pt", padding=True, images=None):
        if images is not None:
            assert all(im.mode == "RGB" for im in images)
            return {"pixel_values": T(np.stack([np.asarray(im.resize((224, 224)), np.float32).transpose(2, 0, 1) / 127.5 - 1.0 for im in images]))}
        return super().__call__(text=text, return_tensors=return_tensors, padding=padding)


def _write_ti_checkpoint(path):
    """stubs.write_synthetic_checkpoint's container with the model of a *_box_text_image checkpoint: text_image PositionNet target and
    tensors, the text_image grounding-tokenizer input, and the VAE encoder (for inpainting)"""
    ck = stubs.write_synthetic_checkpoint(path, TINY, VAE_TINY, max_relations=10)
    content = ck["config_dict"]["_content"]
    content["model"]["params"]["grounding_tokenizer"]["target"] = "ldm.modules.diffusionmodules.text_image_grounding_net.PositionNet"
    content["grounding_tokenizer_input"]["target"] = "grounding_input.text_image_grounding_tokinzer_input.GroundingNetInput"
    ck["model"] = {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in recipe.state_dict(tc.TI_TINY, 0).items()}
    ck["autoencoder"].update({k: T(np.asarray(v)) for k, v in recipe.vae_encoder_state_dict(VAE_TINY, 0).items()})
    torch.save(ck, path)


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt_ti")
    p = str(d / "tiny_gligen_text_image.pth")
    _write_ti_checkpoint(p)
    stubs.install_fake_sng_parser()
    am = itf.load_all_models(p, DEV)
    from PIL import Image
    paths = []
    for i in range(2):
        a = (np.abs(recipe.uniform(f"gputi.img{i}", (40, 56, 3), 4)) * 255).astype(np.uint8)
        paths.append(str(d / f"ref{i}.png"))
        Image.fromarray(a).save(paths[-1])
    P = rnd("proj", (768, 768), 768 ** -0.5)
    return p, am, stubs.toy_clip().to(DEV), _Processor(), paths, P


PROMPTS = ["cat sitting on mat and dog under a tree", "a quiet empty street"]
PHRASES = [[None, "mat"], ["street"]]                   # sample 0: an image-only box and a text-only box; sample 1: text + image
BOXES = [[[0.10, 0.10, 0.50, 0.55], [0.05, 0.60, 0.95, 0.95]], [[0.0, 0.5, 1.0, 1.0]]]


def _expected_conditioning(enc, clip, proc, paths, P):
    """the reference flow (interface.py:114-130, :424-496) restated on the CPU in plain torch"""
    import sng_parser
    from PIL import Image
    images = [[paths[0], None], [paths[1]]]
    g = {k: torch.zeros(2, 30, *s) for k, s in (("boxes", (4,)), ("masks", ()), ("text_masks", ()), ("image_masks", ()),
                                                ("text_embeddings", (768,)), ("image_embeddings", (768,)))}
    for b in range(2):
        for i, (ph, im, loc) in enumerate(zip(PHRASES[b], images[b], BOXES[b])):
            g["boxes"][b, i] = torch.tensor(loc)
            g["masks"][b, i] = 1
            if ph is not None:
                g["text_embeddings"][b, i] = itf.get_clip_feature(clip, proc, ph, "cpu")[0]
                g["text_masks"][b, i] = 1
            if im is not None:
                px = proc(images=[Image.open(im).convert("RGB")])["pixel_values"]
                f = clip.get_image_features(pixel_values=px)
                f = f if torch.is_tensor(f) else f.pooler_output
                y = (f.float() @ P).squeeze(0)
                g["image_embeddings"][b, i] = y / y.norm() * 28.7
                g["image_masks"][b, i] = 1
    rel_ = torch.zeros(2, 10, 768)
    for b, p in enumerate(PROMPTS):
        sg = sng_parser.parse(p)
        trip = [" ".join([sg["entities"][r["subject"]]["lemma_head"], r["relation"], sg["entities"][r["object"]]["lemma_head"]]) for r in sg["relations"]]
        if trip:
            lst = (["PAD"] + trip + trip)[:10]
            rel_[b, :len(lst)] = enc.encode(lst, return_pooler_output=True)[1]
    return dict(context=enc.encode(PROMPTS), uc=enc.encode([""]).repeat(2, 1, 1), relations=rel_, **g)


def _oracle_latent(cond, noise, S, alpha_type, guidance=7.5):
    sd = {k: T(np.asarray(v)).float() for k, v in recipe.state_dict(tc.TI_TINY, 0).items()}
    fc = {k: T(v) for k, v in recipe.sd_first_conv(tc.TI_TINY, 0).items()}
    g = {k: cond[k] for k in KEYS}
    gn = ti_ref.null_grounding(g)
    state = dict(sd=False)

    def eps_fn(x, t, i, alpha):
        if alpha == 0:
            state["sd"] = True
        first = fc if state["sd"] else None
        with torch.no_grad():
            e_c = ti_ref.unet_forward(sd, tc.TI_TINY, x, t, cond["context"], cond["relations"], g, fuser_scale=float(alpha), first_conv=first)
            e_u = ti_ref.unet_forward(sd, tc.TI_TINY, x, t, cond["uc"], cond["relations"], gn, fuser_scale=float(alpha), first_conv=first)
        return e_u + guidance * (e_c - e_u)
    return plms_ref.plms_sample(eps_fn, noise, S, alpha_type)


def test_boundary_run_batch_images_with_reference_images(loaded):
    p, am, clip, proc, paths, P = loaded
    model, autoencoder, text_encoder, diffusion, config = am
    assert isinstance(model.grounding_tokenizer_input, TextImageGroundingNetInput) and model.cfg.grounding == "text_image"
    model.first_conv_type = "GLIGEN"
    torch.manual_seed(123)
    noise = torch.randn(2, 4, 16, 16)
    captured = {}
    dec = autoencoder.decode
    autoencoder.decode = lambda z: dec(captured.setdefault("lat", z.clone()))
    args = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)
    meta = dict(prompts=PROMPTS, phrases=PHRASES, images=[[paths[0], None], [paths[1]]], locations=BOXES, alpha_type=[0.5, 0.0, 0.5],
                projection_matrix=P)
    try:
        imgs = itf.run_batch_images(am, args, meta, noise.to(DEV), clip, proc, device=DEV)
    finally:
        autoencoder.decode = dec
    assert len(imgs) == 2 and imgs[0].size == (32, 32) and imgs[0].mode == "RGB"
    cond = _expected_conditioning(text_encoder.to("cpu"), clip.cpu(), proc, paths, P)
    text_encoder.to(DEV), clip.to(DEV)
    assert cond["image_masks"].sum(-1).tolist() == [1.0, 1.0] and cond["text_masks"].sum(-1).tolist() == [1.0, 1.0]
    lat_ref = _oracle_latent(cond, noise, 4, [0.5, 0.0, 0.5])
    rl = rel_l2(captured["lat"], lat_ref)
    print(f"[ti boundary] latent rel_l2 = {rl:.3e}")
    assert rl < 2.7e-3, rl                               # the bound of test_boundary.py::test_run_batch_images_equals_the_oracle_pipeline
    # inpainting, and a rectangular 16 x 24 latent (image 32 x 48)
    model.first_conv_type = "GLIGEN"
    inp = itf.run_batch_images(am, args, dict(meta, input_image=paths[0]), torch.randn(2, 4, 16, 16).to(DEV), clip, proc, device=DEV)
    assert len(inp) == 2 and inp[0].size == (32, 32)
    model.first_conv_type = "GLIGEN"
    rect = itf.run_batch_images(am, args, meta, torch.randn(2, 4, 16, 24).to(DEV), clip, proc, device=DEV)
    assert len(rect) == 2 and rect[0].size == (48, 32)
    # run_one_image and gligen_inference.run pass the images through
    from layoutllm_t2i_amd import gligen_inference as gi
    gi._MODELS[p] = am
    m1 = dict(ckpt=p, prompt=PROMPTS[0], phrases=None, images=[paths[1]], locations=BOXES[1], projection_matrix=P)
    out = gi.run(m1, dict(batch_size=1, guidance_scale=7.5, no_plms=False, device=DEV, steps=4), starting_noise=torch.randn(1, 4, 16, 16).to(DEV),
                 clip_model=clip, clip_processor=proc)
    assert len(out) == 1 and out[0].size == (32, 32)


def test_images_on_a_text_only_checkpoint_raise(tmp_path, loaded):
    p, am, clip, proc, paths, P = loaded
    pt = str(tmp_path / "text_only.pth")
    stubs.write_synthetic_checkpoint(pt, TINY, VAE_TINY, max_relations=10)
    amt = itf.load_all_models(pt, DEV)
    meta = dict(prompts=PROMPTS, phrases=[["cat", "mat"], ["street"]], images=[[paths[0], None], [None]], locations=BOXES, projection_matrix=P)
    with pytest.raises(ValueError, match="text-only checkpoint"):
        itf.run_batch_images(amt, dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4), meta, torch.randn(2, 4, 16, 16).to(DEV), clip, proc,
                             device=DEV)
