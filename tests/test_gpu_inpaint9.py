"""The inpaint_mode UNet (GLIGEN's checkpoint_inpainting_text*.pth, a 9-channel first conv over cat([x, z0 * mask, mask])) on the GPU: the
two-source pack kernel bit for bit, the first conv against fp64, the tiny UNet against the reference's own outputs (tests/golden/ip9_*.npz)
in default and strict mode, CFG batching with the shared prefix, the extra under graph replay, the masked PLMS run, launch counts, and the
interface boundary on a synthetic 9-channel checkpoint."""
import dataclasses
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import inpaint9_cases as ic
import inpaint9_ref
import stubs
import ti_ref
from layoutllm_t2i_amd import _lib, host, ops, recipe
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import HipLibraryError, init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, TextImageGroundingNetInput, UNetModel
from layoutllm_t2i_amd.weights import pack_first_conv
from test_gpu_inpaint import RecordRandnLike, masked_oracle_loop
from test_gpu_model import rel_l2, report

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
SENT = -999.0


def rnd(tag, shape, scale=1.0):
    return T(recipe.normal(f"gpuip9.{tag}", tuple(shape), 43)) * scale


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


# ------------------------------------------------------------------------------------------- the pack kernel
@pytest.mark.parametrize("h,w", [(3, 4), (8, 8), (8, 16)], ids=["hw12", "hw64", "hw128"])
def test_pack_latent_extra_is_bitwise_the_torch_expression(h, w):
    """gl_pack_latent_extra vs hi = v.half(), lo = (v - hi.float()).half() over cat([x, extra]): B in {1, 2}, reps in {1, 2}, Bs in {1, B},
    split on / off; the padding channels exactly zero, the rows behind the output untouched.  hw = 12: grid-stride tail and indices that
    are no power of two.  x and the masked-latent channels are not fp16-representable; the mask channel is 0 / 1 (lo == 0)."""
    G = 8
    for B in (1, 2):
        x = rnd(f"x{B}.{h}", (B, 4, h, w)) * 1.3
        for Bs in sorted({1, B}):
            extra = rnd(f"e{B}.{Bs}.{h}", (Bs, 5, h, w)) * 0.8
            extra[:, 4] = (extra[:, 4] > 0).float()
            extra[:, :4] *= extra[:, 4:5]
            cat = _nhwc(torch.cat([x, extra.expand(B, -1, -1, -1)], 1))                      # [B * hw, 9]
            hi = cat.half()
            lo = (cat - hi.float()).half()
            assert float(lo[:, :4].abs().max()) > 0 and float(lo[:, 4:8].abs().max()) > 0 and float(lo[:, 8].abs().max()) == 0
            for reps in (1, 2):
                for split in (False, True):
                    rows = reps * B * h * w
                    buf = torch.full((rows + G, 64), SENT, dtype=torch.float16, device=DEV)
                    ops.pack_latent_extra(x.to(DEV), extra.to(DEV), 64, reps, buf[:rows], split=split)
                    got = buf.cpu()
                    want = torch.zeros(B * h * w, 64, dtype=torch.float16)
                    want[:, :9] = hi
                    if split:
                        want[:, 9:18], want[:, 18:27] = lo, hi
                    want = torch.cat([want] * reps, 0)
                    tag = (B, Bs, reps, split)
                    assert torch.equal(got[:rows].view(torch.int16), want.view(torch.int16)), tag      # bit for bit, -0.0 included
                    assert float(got[:rows, 27 if split else 9:].abs().max()) == 0.0, tag
                    assert bool((got[rows:] == SENT).all()), tag


def test_pack_latent_extra_equals_pack_latent_on_the_latent_channels():
    """the first C channels of each part are what the existing kernel writes for the latent alone"""
    x, extra = rnd("px", (2, 4, 8, 8)), rnd("pe", (2, 5, 8, 8))
    a = torch.empty(128, 64, dtype=torch.float16, device=DEV)
    b = torch.empty(128, 64, dtype=torch.float16, device=DEV)
    ops.pack_latent_extra(x.to(DEV), extra.to(DEV), 64, 1, a, split=True)
    ops.pack_latent(x.to(DEV), 64, 1, b, split=True)
    for part in range(3):
        assert torch.equal(a[:, 9 * part:9 * part + 4], b[:, 4 * part:4 * part + 4])


# ------------------------------------------------------------------------------------------- the first conv through HIP
@pytest.mark.parametrize("h,w", [(8, 8), (8, 16)], ids=["8x8", "8x16"])
def test_first_conv_9_channels_vs_fp64(h, w):
    """pack (split) + gl_conv3x3 with weights.pack_first_conv of a [mc, 9, 3, 3] weight vs F.conv2d in fp64 on the UNROUNDED 9-channel input.
    Bar: the error the existing 4-channel split first conv (gl_pack_latent + the same conv kernel) reaches against ITS fp64 reference on the
    same latent and the same weight's first 4 input channels, times 2 for the larger K (27 instead of 12 products per tap)."""
    B, mc = 2, 64
    x = rnd(f"cx{w}", (B, 4, h, w)) * 1.3
    extra = rnd(f"ce{w}", (B, 5, h, w)) * 0.8
    extra[:, 4] = (extra[:, 4] > 0).float()
    w9 = rnd("cw", (mc, 9, 3, 3), 1 / 9)
    b = rnd("cb", (mc,), 0.1)
    xs = torch.empty(B * h * w, 64, dtype=torch.float16, device=DEV)
    out9 = torch.empty(B * h * w, mc, dtype=torch.float32, device=DEV)
    ops.pack_latent_extra(x.to(DEV), extra.to(DEV), 64, 1, xs, split=True)
    ops.conv3x3(xs, pack_first_conv(w9, 64).to(DEV), out9, B, h, w, b.to(DEV))
    ref9 = _nhwc(F.conv2d(torch.cat([x, extra], 1).double(), w9.double(), b.double(), padding=1))
    out4 = torch.empty_like(out9)
    ops.pack_latent(x.to(DEV), 64, 1, xs, split=True)
    ops.conv3x3(xs, pack_first_conv(w9[:, :4].contiguous(), 64).to(DEV), out4, B, h, w, b.to(DEV))
    ref4 = _nhwc(F.conv2d(x.double(), w9[:, :4].double(), b.double(), padding=1))
    e9 = float((out9.cpu().double() - ref9).norm() / ref9.norm())
    e4 = float((out4.cpu().double() - ref4).norm() / ref4.norm())
    print(f"[first_conv_9ch {h}x{w}] rel_l2 vs fp64: 9 channels {e9:.3e}, 4 channels {e4:.3e}, bar {2 * e4:.3e}")
    assert torch.isfinite(out9).all() and e9 <= 2 * e4, (e9, e4)
    assert rel_l2(out9, out4) > 1e-2                                                    # the five extra channels carry weight


# ------------------------------------------------------------------------------------------- whole model: tiny UNet vs the reference
_models = {}


def get_model(family="text", split_weights=False, fresh=False):
    key = (family, split_weights)
    if fresh or key not in _models:
        base = ic.IP_TI_TINY if family == "text_image" else ic.IP_TINY
        m = UNetModel(dataclasses.replace(base, split_weights=split_weights), recipe.state_dict(base, 0), device=DEV)
        m.grounding_tokenizer_input = TextImageGroundingNetInput() if family == "text_image" else GroundingNetInput()
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def _batch(family, inp):
    if family == "text_image":
        return {k: inp[k] for k in ti_ref.KEYS}
    return dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])


def _golden_call(model, case, inp, extra=None):
    model.fuser_scale = case["scale"]
    if case["restore"]:
        model.restore_first_conv_from_SD()                  # switches nothing on an inpaint model
    assert model.first_conv_type == "GLIGEN" and model.use_sd_conv is False
    g = model.grounding_tokenizer_input.prepare(_batch(case["family"], inp))
    d = dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], relations=inp["relations"],
             inpainting_extra_input=inp["extra"] if extra is None else extra, grounding_extra_input=None)
    if case["grounding"] == "real":
        d["grounding_input"] = g
    else:
        d["context"] = inp["uc"]
    return model(d)


@pytest.mark.parametrize("case", ic.UNET_CASES, ids=[c["name"] for c in ic.UNET_CASES])
def test_tiny_unet_matches_reference_golden(case):
    """default mode, the bound tests/test_gpu_ti.py applies to ti_unet_tiny_*; graph replay == eager bitwise; with the extra zeroed the
    output moves by far more than the bound, so it cannot be met with the five channels ignored"""
    model = get_model(case["family"])
    inp = {a: T(v) for a, v in ic.case_inputs(case).items()}
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
    moved = rel_l2(_golden_call(model, case, inp, extra=torch.zeros_like(inp["extra"])), ref)
    print(f"[{case['name']}] extra zeroed: rel_l2 = {moved:.3e}")
    assert moved > 1e-2, moved


@pytest.mark.parametrize("case", ic.UNET_CASES, ids=[c["name"] for c in ic.UNET_CASES])
def test_tiny_unet_strict_matches_reference_golden(case):
    """strict mode on a split_weights handle, the bounds tests/test_gpu_ti.py applies to ti_unet_tiny_* in strict mode"""
    model = get_model(case["family"], True)
    inp = {a: T(v) for a, v in ic.case_inputs(case).items()}
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


def test_model_call_needs_the_extra():
    model = get_model()
    case = ic.by_name("ip9_unet_tiny_s1")
    inp = {a: T(v) for a, v in ic.case_inputs(case).items()}
    g = model.grounding_tokenizer_input.prepare(_batch("text", inp))
    d = dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"]), context=inp["context"], relations=inp["relations"], grounding_input=g,
             inpainting_extra_input=None, grounding_extra_input=None)
    with pytest.raises(ValueError, match="inpainting_extra_input"):
        model(d)
    with pytest.raises(ValueError, match="inpainting_extra_input"):
        model.engine.set_inpaint_extra(torch.zeros(2, 5, 16, 24))


# ------------------------------------------------------------------------------------------- batching
def _cond(eng, inp, ctx_key, null, hw=16):
    z = (lambda t: torch.zeros_like(t)) if null else (lambda t: t)
    eng.set_conditioning(inp[ctx_key], inp["relations"], z(inp["boxes"]), z(inp["masks"]), z(inp["positive_embeddings"]), hw)


def _cond2(eng, inp, hw=16):
    cat = lambda a, b: torch.cat([a, b], 0)
    z = torch.zeros_like
    eng.set_conditioning(cat(inp["context"], inp["uc"]), cat(inp["relations"], inp["relations"]), cat(inp["boxes"], z(inp["boxes"])),
                         cat(inp["masks"], z(inp["masks"])), cat(inp["positive_embeddings"], z(inp["positive_embeddings"])), hw)


@pytest.mark.parametrize("bs", ["per_sample", "broadcast"])
def test_cfg_batched_2b_equals_two_calls(bs):
    """[cond ; uncond] as one 2B batch == two B-sized calls (rel-L2 < 1e-6, as tests/test_gpu_ti.py requires), with the shared cond / uncond
    prefix (option 44) on and off: both halves read the same extra.  Bs = B and Bs = 1 (one extra for every sample)."""
    eng = get_model().engine
    inp = {a: T(v) for a, v in ic.case_inputs(ic.by_name("ip9_unet_tiny_s1")).items()}
    x = inp["x"].to(DEV)
    extra = inp["extra"] if bs == "per_sample" else inp["extra"][1:2]
    _cond(eng, inp, "context", False)
    eng.set_inpaint_extra(extra)
    ec = eng.forward(x, 981.0, 1.0, False, 1).clone()
    _cond(eng, inp, "uc", True)                         # same shape: the extra stays valid
    eu = eng.forward(x, 981.0, 1.0, False, 1).clone()
    assert rel_l2(ec, eu) > 1e-2                        # the two halves are different problems
    _cond2(eng, inp)
    try:
        for share in (1, 0):
            eng.set_option(44, share)
            e2 = eng.forward(x, 981.0, 1.0, False, 2).clone()
            rc, ru = rel_l2(e2[:2], ec), rel_l2(e2[2:], eu)
            print(f"[ip9 2B {bs} share={share}] rel_l2 cond {rc:.2e} uncond {ru:.2e}")
            assert rc < 1e-6 and ru < 1e-6, (share, rc, ru)
    finally:
        eng.clear_options()
    if bs == "broadcast":                               # broadcasting sample 1's extra is not the per-sample extra
        eng.set_inpaint_extra(inp["extra"])
        assert rel_l2(eng.forward(x, 981.0, 1.0, False, 2)[:2], ec) > 1e-3
    with pytest.raises(HipLibraryError, match="inpainting extra has 3 samples"):
        eng.set_inpaint_extra(torch.cat([inp["extra"], inp["extra"][:1]], 0))
        eng.forward(x, 981.0, 1.0, False, 2)
    eng.set_inpaint_extra(inp["extra"])


# ------------------------------------------------------------------------------------------- the extra under graph replay
def test_graph_replay_reads_the_current_extra():
    """the captured graphs read the extra from a fixed pool address at replay time: a new extra needs no new capture and is never stale;
    a conditioning call with another latent shape invalidates it until it is set again (a host-side check, nothing is launched)"""
    m = get_model()
    eng = m.engine
    case = ic.by_name("ip9_unet_tiny_s1")
    inp = {a: T(v) for a, v in ic.case_inputs(case).items()}
    rect = {a: T(v) for a, v in ic.case_inputs(ic.by_name("ip9_unet_tiny_rect")).items()}
    x, xr = inp["x"].to(DEV), rect["x"].to(DEV)
    e1 = inp["extra"]
    e2 = torch.cat([e1[1:], e1[:1]], 0) * torch.tensor([0.5, 0.5, 0.5, 0.5, 1.0]).view(1, 5, 1, 1)
    assert eng.use_graphs
    _cond(eng, inp, "context", False)
    eng.set_inpaint_extra(e1)
    eng.forward(x, 601.0, 1.0, False, 1)                # captures (or replays) ...
    r1 = eng.forward(x, 601.0, 1.0, False, 1).clone()   # ... and this one is a pure replay
    eng.set_inpaint_extra(e2)
    r2 = eng.forward(x, 601.0, 1.0, False, 1).clone()   # replay with the second extra

    def fresh_eager(inp_, x_, extra, hw):
        f = get_model(fresh=True)
        f.engine.use_graphs = False
        _cond(f.engine, inp_, "context", False, hw)
        f.engine.set_inpaint_extra(extra)
        return f.engine.forward(x_, 601.0, 1.0, False, 1).clone()
    assert torch.equal(r2, fresh_eager(inp, x, e2, 16)), "replay after set_inpaint_extra == eager forward of a fresh handle"
    assert not torch.equal(r2, r1) and rel_l2(r2, r1) > 1e-3
    # a conditioning call of another shape in between
    _cond(eng, rect, "context", False, (8, 16))
    with pytest.raises(HipLibraryError, match="gl_set_inpaint_extra"):
        eng.forward(xr, 601.0, 1.0, False, 1)
    with pytest.raises(ValueError, match="inpainting_extra_input"):
        eng.set_inpaint_extra(e1)                       # the old shape is refused by the Python face
    eng.set_inpaint_extra(rect["extra"])
    eng.forward(xr, 601.0, 1.0, False, 1)
    rr = eng.forward(xr, 601.0, 1.0, False, 1).clone()
    assert torch.equal(rr, fresh_eager(rect, xr, rect["extra"], (8, 16)))
    _cond(eng, inp, "context", False)
    with pytest.raises(HipLibraryError, match="gl_set_inpaint_extra"):
        eng.forward(x, 601.0, 1.0, False, 1)
    eng.set_inpaint_extra(e1)
    assert torch.equal(eng.forward(x, 601.0, 1.0, False, 1), r1)
    # sd_conv on an inpaint handle: refused by the Python face and by the C entry
    with pytest.raises(RuntimeError, match="SD first-conv"):
        eng.forward(x, 601.0, 1.0, True, 1)
    eps = torch.empty(2, 4, 16, 16, device=DEV)
    assert eng._lib.gl_unet_forward(eng.handle, x.data_ptr(), None, 601.0, 1, 1.0, 1, eps.data_ptr(), 0, None) == -1
    assert "sd_conv != 0 on an inpaint_mode handle" in _lib.last_error(eng.handle)
    # the entry on a text handle
    tx = UNetModel(TINY, recipe.state_dict(TINY, 0), device=DEV)
    with pytest.raises(ValueError, match="without inpaint_mode"):
        tx.engine.set_inpaint_extra(e1)
    ed = e1.to(DEV)
    assert tx.engine._lib.gl_set_inpaint_extra(tx.engine.handle, ed.data_ptr(), 2, None) == -1 and "inpaint_mode = 0" in _lib.last_error(tx.engine.handle)


# ------------------------------------------------------------------------------------------- launch counts
def test_launch_count_equals_a_text_handle():
    """the two-source pack takes the place of gl_pack_latent: an inpaint handle's forward has as many launches as a text handle's"""
    ip, tx = get_model().engine, UNetModel(TINY, recipe.state_dict(TINY, 0), device=DEV).engine
    inp = {a: T(v) for a, v in ic.case_inputs(ic.by_name("ip9_unet_tiny_s1")).items()}
    x = inp["x"].to(DEV)
    for reps in (1, 2):
        for eng in (ip, tx):
            (_cond2 if reps == 2 else lambda e, i: _cond(e, i, "context", False))(eng, inp)
        ip.set_inpaint_extra(inp["extra"])
        for scale in (1.0, 0.0):
            counts = []
            for eng in (ip, tx):
                eng.use_graphs = False
                try:
                    eng.forward(x, 501.0, scale, False, reps)
                finally:
                    eng.use_graphs = True
                counts.append(eng.num_launches())
            print(f"[ip9 launches reps={reps} fuser={'on' if scale else 'off'}] inpaint {counts[0]} text {counts[1]}")
            assert counts[0] == counts[1] > 0, (reps, scale, counts)


# ------------------------------------------------------------------------------------------- PLMS
def test_masked_plms_matches_reference_golden():
    """the 10-step golden (CFG 7.5, mask and x0, the extra, B = 2, alpha_type [0.3, 0, 0.7]: seven scale-0 steps) through PLMSSampler, the
    bound of tests/test_gpu_inpaint.py::test_masked_sampler_matches_reference_golden; no conv switch happens"""
    case = ic.by_name("ip9_plms_tiny")
    raw = ic.case_inputs(case)
    inp = {a: T(v) for a, v in raw.items() if isinstance(v, np.ndarray)}
    model = get_model()
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
    with RecordRandnLike(replay=raw["noises"]) as rec:
        out = itf.denoise((model, None, None, LatentDiffusion(device=DEV), {}), inp["context"], inp["uc"], inp["relations"], batch,
                          inp["x"].to(DEV), case["alpha_type"], case["guidance"], steps=case["S"], mask=inp["mask"].to(DEV), x0=inp["x0"].to(DEV),
                          inpainting_extra_input=inp["extra"])
    assert rec.shapes == raw["draw_shapes"].tolist()
    assert model.first_conv_type == "GLIGEN" and model.use_sd_conv is False and model.fuser_scale == 0
    r = rel_l2(out, T(np.load(os.path.join(GOLD, "ip9_plms_tiny.npz"))["out"]))
    print(f"[ip9_plms_tiny] rel_l2={r:.3e}")
    assert torch.isfinite(out).all() and r < 3.1e-3, r
    with pytest.raises(ValueError, match="inpainting_extra_input"):
        itf.denoise((model, None, None, LatentDiffusion(device=DEV), {}), inp["context"], inp["uc"], inp["relations"], batch, inp["x"].to(DEV),
                    case["alpha_type"], case["guidance"], steps=2, mask=inp["mask"].to(DEV), x0=inp["x0"].to(DEV))


# ------------------------------------------------------------------------------------------- the boundary
def _write_checkpoint(path, family="text", inpaint=True):
    """stubs.write_synthetic_checkpoint's container as GLIGEN's inpainting checkpoints have it: ``inpaint_mode: True``, a [mc, 9, 3, 3] first
    conv, the VAE encoder, and no SD conv file next to it"""
    ck = stubs.write_synthetic_checkpoint(path, TINY, VAE_TINY, max_relations=10, with_sd_conv=not inpaint)
    content = ck["config_dict"]["_content"]
    cfg = dataclasses.replace(TINY, grounding=family, inpaint_mode=inpaint)
    if inpaint:
        content["model"]["params"]["inpaint_mode"] = True
    if family == "text_image":
        content["model"]["params"]["grounding_tokenizer"]["target"] = "ldm.modules.diffusionmodules.text_image_grounding_net.PositionNet"
        content["grounding_tokenizer_input"]["target"] = "grounding_input.text_image_grounding_tokinzer_input.GroundingNetInput"
    ck["model"] = {k: torch.tensor(np.asarray(v, dtype=np.float32)) for k, v in recipe.state_dict(cfg, 0).items()}
    ck["autoencoder"].update({k: T(np.asarray(v)) for k, v in recipe.vae_encoder_state_dict(VAE_TINY, 0).items()})
    torch.save(ck, path)
    return cfg


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt_inpaint9")
    p = str(d / "tiny_gligen_inpainting_text.pth")
    _write_checkpoint(p)
    stubs.install_fake_sng_parser()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        am = itf.load_all_models(p, DEV)
    assert not any("SD_input_conv" in str(w.message) for w in caught), "an inpaint checkpoint neither looks for the SD conv nor misses it"
    return p, am, stubs.toy_clip().to(DEV), stubs.ToyProcessor(), d


def _input_image():
    from PIL import Image
    a = (np.clip(recipe.uniform("gpuip9.img", (40, 56, 3), 4), 0, 1) * 255).astype(np.uint8)
    return Image.fromarray(a)


LOC = [[0.10, 0.10, 0.50, 0.55], [0.55, 0.20, 0.90, 0.70]]
ARGS = dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4)


def test_run_one_image_matches_the_mirror_pipeline(loaded):
    p, am, clip, proc, d = loaded
    model, autoencoder, text_encoder, diffusion, config = am
    assert model.cfg.inpaint_mode and model.cfg.first_conv_in == 9 and not model.first_conv_restorable and not model.engine.P.has_sd_conv
    assert "sd_first_conv.w" not in model.engine.W
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5], input_image=_input_image())
    seen, captured = {}, {}
    orig, dec = itf.denoise, autoencoder.decode

    def spy(*a, **k):
        seen["a"], seen["k"] = a, k
        return orig(*a, **k)
    itf.denoise = spy
    autoencoder.decode = lambda z: dec(captured.setdefault("lat", z.clone()))
    try:
        torch.manual_seed(31)
        noise = torch.randn(2, 4, 16, 16)
        with RecordRandnLike() as rec:
            imgs = itf.run_one_image(am, dict(ARGS), meta, noise.to(DEV), clip, proc, device=DEV)
    finally:
        itf.denoise, autoencoder.decode = orig, dec
    assert len(imgs) == 2 and all(im.size == (32, 32) and im.mode == "RGB" for im in imgs)
    context, uc, relations, batch = (seen["a"][i] for i in range(1, 5))
    mask, z0, extra = seen["k"]["mask"], seen["k"]["x0"], seen["k"]["inpainting_extra_input"]
    assert torch.equal(mask.cpu(), host.draw_masks_from_boxes(batch["boxes"], 16)) and tuple(z0.shape) == (1, 4, 16, 16)
    assert tuple(extra.shape) == (2, 5, 16, 16) and torch.equal(extra, torch.cat([z0 * mask, mask], 1))
    assert model.first_conv_type == "GLIGEN"            # alpha_type [0.5, 0, 0.5] ran scale-0 steps: nothing was switched
    # the mirror pipeline on the CPU: tests/inpaint9_ref.py inside the masked PLMS loop, fed the same z0, mask and q_sample noises
    q_noises = [rec.values[j] for j in range(len(rec.values)) if j == 0 or (j >= 3 and (j - 3) % 2 == 0)]
    assert len(q_noises) == 4 and all(tuple(n.shape) == (1, 4, 16, 16) for n in q_noises)
    sd = {k: T(np.asarray(v)).float() for k, v in recipe.state_dict(ic.IP_TINY, 0).items()}
    c = lambda t: t.detach().float().cpu()
    g = dict(boxes=c(batch["boxes"]), masks=c(batch["masks"]), positive_embeddings=c(batch["text_embeddings"]))
    gn = inpaint9_ref.null_grounding(g)
    ex = c(extra)

    def eps_fn(x, t, i, alpha):
        with torch.no_grad():
            e_c = inpaint9_ref.unet_forward(sd, ic.IP_TINY, x, ex, t, c(context), c(relations), g, fuser_scale=float(alpha))
            e_u = inpaint9_ref.unet_forward(sd, ic.IP_TINY, x, ex, t, c(uc), c(relations), gn, fuser_scale=float(alpha))
        return e_u + 7.5 * (e_c - e_u)
    lat_ref = masked_oracle_loop(eps_fn, noise, 4, [0.5, 0.0, 0.5], z0, mask, q_noises, diffusion)
    rl = rel_l2(captured["lat"], lat_ref)
    print(f"[ip9 boundary] latent rel_l2 = {rl:.3e}")
    assert rl < 2.7e-3, rl                              # the bound of tests/test_gpu_ti.py's boundary test


def test_every_entry_point_inpaints(loaded, tmp_path):
    """run_batch_images (one image per sample), gligen_inference.run, a rectangular starting noise, and the refusals"""
    p, am, clip, proc, d = loaded
    img = _input_image()
    path = str(tmp_path / "in.png")
    img.save(path)
    metab = dict(prompts=["cat sitting on mat", "a quiet street"], phrases=[["cat"], ["street"]],
                 locations=[[[0.1, 0.1, 0.5, 0.5]], [[0.0, 0.5, 1.0, 1.0]]], alpha_type=[0.5, 0.0, 0.5], input_image=[img, path])
    imgs = itf.run_batch_images(am, dict(ARGS), metab, torch.randn(2, 4, 16, 16).to(DEV), clip, proc, device=DEV)
    assert len(imgs) == 2 and imgs[0].size == (32, 32)
    rect = itf.run_batch_images(am, dict(ARGS), metab, torch.randn(2, 4, 8, 16).to(DEV), clip, proc, device=DEV)
    assert len(rect) == 2 and rect[0].size == (32, 16)
    from layoutllm_t2i_amd import gligen_inference as gi
    gi._MODELS[p] = am
    m1 = dict(ckpt=p, prompt="cat sitting on mat", phrases=["cat"], locations=[[0.1, 0.1, 0.5, 0.5]], save_folder_name="ip9", input_image=path)
    cfg = dict(batch_size=1, guidance_scale=7.5, no_plms=False, folder=str(tmp_path), device=DEV, steps=4)
    out = gi.run(m1, cfg, starting_noise=torch.randn(1, 4, 16, 16).to(DEV), clip_model=clip, clip_processor=proc)
    assert len(out) == 1 and out[0].size == (32, 32) and os.path.exists(tmp_path / "ip9" / "0.png")
    with pytest.raises(ValueError, match="input_image"):
        gi.run({k: v for k, v in m1.items() if k != "input_image"}, cfg, starting_noise=torch.randn(1, 4, 16, 16).to(DEV), clip_model=clip,
               clip_processor=proc)
    with pytest.raises(ValueError, match="input_image"):
        itf.run_batch_images(am, dict(ARGS), {k: v for k, v in metab.items() if k != "input_image"}, torch.randn(2, 4, 16, 16).to(DEV), clip, proc,
                             device=DEV)


def test_strict_and_text_image_inpainting_checkpoints(loaded, tmp_path):
    p, am, clip, proc, d = loaded
    img = _input_image()
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5], input_image=img)
    ams = itf.load_all_models(p, DEV, strict=True)
    assert ams[0].strict and ams[0].cfg.split_weights and ams[0].cfg.inpaint_mode
    torch.manual_seed(5)
    noise = torch.randn(2, 4, 16, 16).to(DEV)
    lat = {}
    for tag, models in (("strict", ams), ("default", am)):
        dec = models[1].decode
        models[1].decode = lambda z, dec=dec, tag=tag: dec(lat.setdefault(tag, z.clone()))
        try:
            torch.manual_seed(6)
            out = itf.run_one_image(models, dict(ARGS), meta, noise.clone(), clip, proc, device=DEV)
        finally:
            models[1].decode = dec
        assert len(out) == 2 and out[0].size == (32, 32)
    r = rel_l2(lat["default"], lat["strict"])
    print(f"[ip9 boundary] default vs strict latent rel_l2 = {r:.3e}")
    # the default-mode latent is within 2.7e-3 of the fp32 mirror (the boundary bound above) and the strict-mode one within 1e-4 of it (twice
    # the per-forward strict bound 5e-5 over these 5 evaluations' accumulated effect is still below that): the two differ by less than the sum
    assert 0 < r < 2.7e-3 + 1e-4, r
    # a text_image inpainting checkpoint (checkpoint_inpainting_text_image.pth's layout), with a reference image on one box
    pt = str(tmp_path / "tiny_gligen_inpainting_text_image.pth")
    _write_checkpoint(pt, family="text_image")
    amt = itf.load_all_models(pt, DEV)
    assert amt[0].cfg.grounding == "text_image" and amt[0].cfg.inpaint_mode and isinstance(amt[0].grounding_tokenizer_input, TextImageGroundingNetInput)
    ref_img = str(tmp_path / "ref.png")
    img.save(ref_img)
    from test_gpu_ti import _Processor
    P = rnd("proj", (768, 768), 768 ** -0.5)
    mti = dict(meta, phrases=[None, "mat"], images=[ref_img, None], projection_matrix=P)
    out = itf.run_one_image(amt, dict(ARGS), mti, torch.randn(2, 4, 16, 16).to(DEV), clip, _Processor(), device=DEV)
    assert len(out) == 2 and out[0].size == (32, 32)


def test_four_channel_checkpoint_keeps_the_latent_blend_path(tmp_path):
    """the same synthetic checkpoint without inpaint_mode and with 4-channel weights: no extra is built, the sampler blends the latent"""
    p = str(tmp_path / "tiny_gligen_text.pth")
    cfg = _write_checkpoint(p, inpaint=False)
    assert not cfg.inpaint_mode
    stubs.install_fake_sng_parser()
    am = itf.load_all_models(p, DEV)
    assert not am[0].cfg.inpaint_mode and am[0].first_conv_restorable and "sd_first_conv.w" in am[0].engine.W
    seen = {}
    orig = itf.denoise

    def spy(*a, **k):
        seen["k"] = k
        return orig(*a, **k)
    itf.denoise = spy
    try:
        meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5], input_image=_input_image())
        imgs = itf.run_one_image(am, dict(ARGS), meta, torch.randn(2, 4, 16, 16).to(DEV), stubs.toy_clip().to(DEV), stubs.ToyProcessor(), device=DEV)
    finally:
        itf.denoise = orig
    assert len(imgs) == 2 and imgs[0].size == (32, 32)
    assert seen["k"]["inpainting_extra_input"] is None and seen["k"]["mask"] is not None and seen["k"]["x0"] is not None
    assert am[0].first_conv_type == "SD"                # the 4-channel model still switches its conv on the scale-0 steps
    # ... and no input image is no error on such a model
    meta.pop("input_image")
    am[0].first_conv_type = "GLIGEN"
    assert len(itf.run_one_image(am, dict(ARGS), meta, torch.randn(2, 4, 16, 16).to(DEV), stubs.toy_clip().to(DEV), stubs.ToyProcessor(), device=DEV)) == 2
