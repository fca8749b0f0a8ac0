"""Rectangular (h != w) latents on a real MI355X: the reference's rectangular goldens through the HIP path, square shapes through
the new entries against the old ones (bitwise), graph replay and alternating shapes on one handle, the full-size UNet and VAE at
64 x 96 / 96 x 64 against the oracle, the conv forms at non-square maps, and the interface end to end on the synthetic checkpoint.

Every bound is the one the matching SQUARE test uses (imported where the module can be imported, restated with its origin otherwise);
both orientations run wherever a transposed-shape bug could hide behind one.

st_rect (a bare SpatialTransformer) has no entry of its own on the HIP side, as st_64 has none: the engine runs whole UNets.  It pins the
oracle in tests/test_rect_host.py; on the GPU the transformer blocks at h != w are reached through the unet_tiny_rect_* goldens (three
levels of them, both orientations, fuser on and off) and the full-size cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import rect_cases as rc
import stubs
import test_gpu_configs as tgc
import test_gpu_inpaint as tgi
import vae_encoder_pyref
from layoutllm_t2i_amd import _lib, arch, host, ops, recipe
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd._lib import EPI_GATE_RES, EPI_GEGLU, init_device
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, VAEConfig
from layoutllm_t2i_amd.interface import denoise
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel
from layoutllm_t2i_amd.vae import VAEDecoder, VAEEncoder
from layoutllm_t2i_amd.weights import geglu_interleave, pack_conv3x3
from oracle import vae_ref

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
PARITY_OUT = os.environ.get("RECT_PARITY_OUT")      # a file that collects the measured values (profiles/rect_parity.txt was made this way)

# bounds of the square twins
TINY_UNET_BOUND = 2.1e-3        # test_gpu_model.test_tiny_unet_matches_reference_golden
PLMS_TINY_BOUND = 3.1e-3        # test_gpu_model.test_plms_tiny_matches_reference_golden, test_gpu_inpaint.test_masked_sampler_matches_reference_golden
VAE_BOUND = 6e-3                # test_gpu_vae (tiny golden and full size), test_gpu_inpaint (encoder: tiny golden and full size)
RELA_BOUND = (3e-4, 2e-3)       # test_gpu_kernels.test_rela_fuse_reference_goldens_through_hip: rel-L2, max |err|
CONV_BOUND = (1e-3, 1e-2)       # test_gpu_inpaint.test_conv3x3_pad01_matches_padded_conv: rel-L2, max |err| / max |ref|
BOUND_FULL, FRAC_FULL = tgc.BOUND_FULL, tgc.FRAC_FULL           # test_gpu_configs.py:130-131 (8.1e-4, 0.32)
STRICT_FRAC, STRICT_L2 = 0.001, 3e-5                            # test_gpu_configs.py:212 ff.


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def note(line):
    """measured values: printed, and appended to $RECT_PARITY_OUT when that is set"""
    print(line)
    if PARITY_OUT:
        with open(PARITY_OUT, "a") as f:
            f.write(line + "\n")


_tiny = {}


def tiny_model(strict=False):
    if strict not in _tiny:
        import dataclasses
        cfg = dataclasses.replace(TINY, split_weights=True) if strict else TINY
        m = UNetModel(cfg, recipe.state_dict(TINY, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(TINY, 0))
        if strict:
            m.set_strict(True)
        m.grounding_tokenizer_input = GroundingNetInput()
        _tiny[strict] = m
    return _tiny[strict]


def tiny_inputs(hw, seed=4321, B=2):
    return {k: T(v) for k, v in recipe.synth_inputs(TINY, B, hw, n_boxes=4, n_rel=3, seed=seed).items()}


def set_cond(eng, inp, hw):
    eng.set_conditioning(inp["context"], inp["relations"], inp["boxes"], inp["masks"], inp["positive_embeddings"], hw)


# ------------------------------------------------------------------------------------------- 1. reference goldens through HIP
@pytest.mark.parametrize("name", ["rela_rect_wide", "rela_rect_tall"])
def test_rela_rect_goldens_through_hip(name):
    """test_gpu_kernels.test_rela_fuse_reference_goldens_through_hip's chain (LN3 + stats -> rela_pool -> LN1 -> q GEMM -> attention over
    the relation tokens -> gated o-proj -> LN2 -> GEGLU FF -> gated ff2 -> rela_merge; module output = 2 y - x) at h != w."""
    case = rc.case(name)
    h, w = case["h"], case["w"]
    inp = {a: T(v) for a, v in rc.case_inputs(case).items()}
    Cc, heads, mo = case["C"], case["heads"], 30
    d = Cc // heads
    sd = {n: T(np.asarray(recipe.tensor(f"golden.{name}.{n}", shp, 0))) for n, shp in arch.rela_params("", Cc, rc.CTX).items()}
    dv = lambda t: t.float().contiguous().to(DEV)
    hd = lambda t: t.to(torch.float16).contiguous().to(DEV)
    B, R = inp["x"].shape[0], inp["relations"].shape[1]
    N = h * w
    rects, nvalid, poison = host.box_rects(inp["boxes"].numpy(), inp["masks"].numpy(), h, w)
    dr, dn, dp = (T(a).to(DEV) for a in (rects, nvalid, poison))
    x = inp["x"].reshape(B * N, Cc)
    xd = dv(x)
    e16 = lambda *shape: torch.empty(*shape, dtype=torch.float16, device=DEV)
    st = torch.empty(B * N, 2, dtype=torch.float32, device=DEV)
    hid = ops.layernorm(xd, e16(B * N, Cc), dv(sd["norm3.weight"]), dv(sd["norm3.bias"]), B, N, stats=st)
    fn = e16(B * mo, Cc)
    feat = ops.rela_pool(hid, B, h, w, Cc, dr, dn, dp, mo, e16(B * mo, Cc), ln_gamma=dv(sd["norm1.weight"]), ln_beta=dv(sd["norm1.bias"]), ln_out=fn)
    q = ops.gemm(fn, hd(sd["attn.to_q.weight"]), e16(B * mo, Cc))
    kv = ops.gemm(hd(inp["relations"].reshape(B * R, -1)), hd(torch.cat([sd["attn.to_k.weight"], sd["attn.to_v.weight"]], 0)), e16(B * R, 2 * Cc))
    vt = torch.zeros(B, heads, d, ops.vt_ld(R), dtype=torch.float16, device=DEV)
    ops.transpose_v(kv[:, Cc:], R * 2 * Cc, 2 * Cc, vt, B, heads, d, R)
    ar = e16(B * mo, Cc)
    ops.attention(q, mo * Cc, Cc, kv, R * 2 * Cc, 2 * Cc, vt, ar, mo * Cc, Cc, B, heads, d, mo, R, d ** -0.5)
    ga = torch.tanh(sd["alpha_attn"]).reshape(1).float().to(DEV)
    gdn = torch.tanh(sd["alpha_dense"]).reshape(1).float().to(DEV)
    f1 = ops.gemm(ar, hd(sd["attn.to_out.0.weight"]), e16(B * mo, Cc), dv(sd["attn.to_out.0.bias"]), EPI_GATE_RES, res=feat, gate=ga)
    fn2 = ops.layernorm(f1, e16(B * mo, Cc), dv(sd["norm2.weight"]), dv(sd["norm2.bias"]), B, mo)
    hg = ops.gemm(fn2, hd(geglu_interleave(sd["ff.net.0.proj.weight"])), e16(B * mo, 4 * Cc), dv(geglu_interleave(sd["ff.net.0.proj.bias"])), EPI_GEGLU)
    f2 = ops.gemm(hg, hd(sd["ff.net.2.weight"]), e16(B * mo, Cc), dv(sd["ff.net.2.bias"]), EPI_GATE_RES, res=f1, gate=gdn)
    y = torch.empty(B * N, Cc, dtype=torch.float32, device=DEV)
    ops.rela_merge(xd, None, f2, B, h, w, Cc, dr, dn, dp, mo, y, ln_stats=st, gamma=dv(sd["norm3.weight"]), beta=dv(sd["norm3.bias"]))
    out = (2.0 * y.cpu() - x).view(B, N, Cc)
    ref = T(gold(name)["out"])
    assert torch.isfinite(out).all() and torch.isfinite(ref).all()
    err = (out - ref).abs()
    rl2 = rel_l2(out, ref)
    note(f"[{name}] {h}x{w} rel_l2={rl2:.3e} max|err|={float(err.max()):.3e}")
    assert rl2 < RELA_BOUND[0] and float(err.max()) < RELA_BOUND[1], (rl2, float(err.max()))


def _conv_vs_ref(xd, w, b, B, h, w_, ref_nchw, name, **kw):
    Cout = w.shape[0]
    oh, ow = ref_nchw.shape[-2:]
    out = torch.empty(B * oh * ow, Cout, dtype=torch.float32, device=DEV)
    if kw.pop("pad01", False):
        ops.conv3x3_pad01(xd, pack_conv3x3(w.to(DEV)), out, B, h, w_, b.to(DEV))
    else:
        ops.conv3x3(xd, pack_conv3x3(w.to(DEV)), out, B, h, w_, b.to(DEV), **kw)
    torch.cuda.synchronize()
    got = out.cpu().reshape(B, oh, ow, Cout).permute(0, 3, 1, 2)
    r, err = rel_l2(got, ref_nchw), float((got - ref_nchw).abs().max())
    note(f"[{name}] {h}x{w_} -> {oh}x{ow} rel_l2={r:.3e} max|err|={err:.3e}")
    assert torch.isfinite(got).all() and r < CONV_BOUND[0] and err < CONV_BOUND[1] * float(ref_nchw.abs().max()), (name, r, err)


@pytest.mark.parametrize("name", ["down_rect", "up_rect"])
def test_down_up_rect_goldens_through_hip(name):
    """Downsample (stride-2 conv) 8 x 12 -> 4 x 6 and Upsample (nearest 2x + conv) 4 x 6 -> 8 x 12 of the reference, through gl_conv3x3 with
    an fp32 output.  The golden is fp32 on unrounded operands: fp16 rounding of activations and weights (relative error uniform in
    +-2^-11, rms 2.8e-4 each, independent over the 576 products) puts the result at rel-L2 ~4e-4 -- inside the 1e-3 the conv tests of
    test_gpu_inpaint.py use against an fp32 conv."""
    init_device()
    case = rc.case(name)
    h, w, B, Cc = case["h"], case["w"], case["B"], case["C"]
    x = T(rc.case_inputs(case)["x"])
    key = "op" if name == "down_rect" else "conv"
    sd = {n: T(np.asarray(recipe.tensor(f"golden.{name}.{n}", s, 0))) for n, s in arch.conv_params(key, Cc, Cc).items()}
    xd = x.permute(0, 2, 3, 1).reshape(B * h * w, Cc).half().to(DEV).contiguous()
    ref = T(gold(name)["out"])
    assert tuple(ref.shape[-2:]) == ((h // 2, w // 2) if name == "down_rect" else (2 * h, 2 * w))
    kw = dict(stride=2) if name == "down_rect" else dict(upsample2x=True)
    _conv_vs_ref(xd, sd[key + ".weight"], sd[key + ".bias"], B, h, w, ref, name, **kw)


@pytest.mark.parametrize("name", ["unet_tiny_rect_wide", "unet_tiny_rect_tall"])
def test_tiny_unet_rect_matches_reference_golden(name):
    case = rc.case(name)
    model = tiny_model()
    inp = {a: T(v) for a, v in rc.case_inputs(case).items()}
    model.fuser_scale = case["scale"]
    model.first_conv_type = "SD" if case["sdconv"] else "GLIGEN"
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
    g = model.grounding_tokenizer_input.prepare(batch, None)
    d = dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], relations=inp["relations"],
             inpainting_extra_input=None, grounding_extra_input=None, grounding_input=g)
    try:
        out = model(d)
    finally:
        model.fuser_scale, model.first_conv_type = 1.0, "GLIGEN"
    ref = T(gold(name)["out"])
    assert tuple(out.shape) == tuple(ref.shape) == (2, 4, case["h"], case["w"]) and torch.isfinite(out).all()
    r = rel_l2(out, ref)
    note(f"[{name}] rel_l2={r:.3e} max|err|={float((out.cpu() - ref).abs().max()):.3e}")
    assert r < TINY_UNET_BOUND, r
    # the transposed latent is a different problem, not the same one in another layout
    assert model.engine.cond["H"] == case["h"] and model.engine.cond["W"] == case["w"]


def test_vae_tiny_rect_matches_reference_golden():
    case = rc.case("vae_tiny_rect")
    z = T(rc.case_inputs(case)["z"])
    dec = VAEDecoder(recipe.vae_state_dict(VAE_TINY, 0), VAE_TINY, DEV)
    out = dec.decode(z)
    ref = T(gold("vae_tiny_rect")["out"])
    assert tuple(out.shape) == tuple(ref.shape) == (2, 3, 16, 24) and out.dtype == torch.float32
    r = rel_l2(out, ref)
    note(f"[vae_tiny_rect] rel_l2={r:.3e}")
    assert torch.isfinite(out).all() and r < VAE_BOUND, r
    assert torch.equal(out, dec.decode_oplevel(z)) and torch.equal(out, dec.decode(z))


def test_tiny_encoder_rect_matches_reference_golden():
    g = gold("vae_enc_tiny_rect")
    enc = VAEEncoder(tgi.enc_sd(VAE_TINY), VAE_TINY, DEV)
    z = enc.encode(T(g["x"]), T(g["noise"]))
    zo, mean = enc.encode_oplevel(T(g["x"]), T(g["noise"]), return_mean=True)
    assert tuple(z.shape) == g["z"].shape == (2, 4, 16, 24) and torch.isfinite(z).all()
    rz, rm = rel_l2(z, T(g["z"])), rel_l2(mean, T(g["mean"]))
    note(f"[vae_enc_tiny_rect] rel_l2 z={rz:.3e} mean={rm:.3e}")
    assert rz < VAE_BOUND and rm < VAE_BOUND, (rz, rm)
    assert torch.equal(z, zo) and torch.equal(z, enc.encode(T(g["x"]), T(g["noise"])))


def _run_plms(model, case, inp, mask=None, x0=None):
    model.first_conv_type = "GLIGEN"
    batch = dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"])
    return denoise((model, None, None, LatentDiffusion(device=DEV), {}), inp["context"], inp["uc"], inp["relations"], batch, inp["x"].to(DEV),
                   case["alpha_type"], case["guidance"], steps=case["S"], mask=mask, x0=x0)


def test_plms_rect_tiny_matches_reference_golden():
    case = rc.case("plms_rect_tiny")
    model = tiny_model()
    inp = {a: T(v) for a, v in rc.case_inputs(case).items()}
    out = _run_plms(model, case, inp)
    assert model.first_conv_type == "SD"
    ref = T(gold("plms_rect_tiny")["out"])
    assert tuple(out.shape) == tuple(ref.shape) == (2, 4, 16, 24)
    r = rel_l2(out, ref)
    note(f"[plms_rect_tiny] rel_l2={r:.3e}")
    assert torch.isfinite(out).all() and r < PLMS_TINY_BOUND, r


def test_masked_sampler_rect_matches_reference_golden():
    case = rc.case("plms_inpaint_rect_tiny")
    model = tiny_model()
    inp = {a: T(v) for a, v in rc.case_inputs(case).items()}
    g = gold("plms_inpaint_rect_tiny")
    mask = T(g["mask"]).to(DEV)
    assert torch.equal(host.draw_masks_from_boxes(inp["boxes"], (16, 24)), T(g["mask"]))
    noises = [g[f"noise_{i:03d}"] for i in range(len(g["draw_shapes"]))]
    with tgi.RecordRandnLike(replay=noises) as rec:
        out = _run_plms(model, case, inp, mask, T(g["x0"]).to(DEV))
    assert rec.shapes == g["draw_shapes"].tolist()
    r = rel_l2(out, T(g["out"]))
    note(f"[plms_inpaint_rect_tiny] rel_l2={r:.3e}")
    assert tuple(out.shape) == (2, 4, 16, 24) and torch.isfinite(out).all() and r < PLMS_TINY_BOUND, r


# ------------------------------------------------------------------------------------------- 2. square: new entries == old entries
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
def test_square_through_hw_entry_equals_old_entry_unet(strict):
    model = tiny_model(strict)
    eng = model.engine
    inp = tiny_inputs(16)
    x = inp["x"].to(DEV)
    outs = {}
    for graphs in (True, False):
        eng.use_graphs = graphs
        try:
            for key, hw in (("old", 16), ("new", (16, 16)), ("old2", 16)):
                set_cond(eng, inp, hw)
                outs[key, graphs] = (eng.forward(x, 481.0, 1.0, False, 1).clone(), eng.forward(x, 201.0, 0.0, True, 1).clone(), eng.num_launches())
        finally:
            eng.use_graphs = True
    ref = outs["old", True]
    assert torch.isfinite(ref[0]).all()
    for key, val in outs.items():
        assert torch.equal(val[0], ref[0]) and torch.equal(val[1], ref[1]), key
    assert len({v[2] for v in outs.values()}) == 1                      # the same launch sequence
    # the C entry itself: h == w through gl_set_conditioning_hw is accepted whatever gl_set_conditioning accepts at a multiple of 8, and a
    # shape that breaks the rule comes back as GL_ERR_BAD_ARG without touching the handle's conditioning
    f32 = lambda t: t.float().contiguous().to(DEV)
    c = [f32(inp[k]) for k in ("context", "relations", "boxes", "masks", "positive_embeddings")]
    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for bad in ((12, 20), (16, 20), (0, 16), (16, -8)):
        assert l.gl_set_conditioning_hw(eng.handle, *[t.data_ptr() for t in c], 2, 77, 10, bad[0], bad[1], st) == -1
    assert torch.equal(eng.forward(x, 481.0, 1.0, False, 1), ref[0])


def test_square_through_hw_entries_equals_old_entries_vae():
    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    dec = VAEDecoder(tgi.enc_sd(VAE_TINY), VAE_TINY, DEV)
    z = (T(recipe.normal("rect.sq.z", (2, 4, 8, 8), 3)) * np.float32(0.18215)).to(DEV)
    old = dec.decode(z)                                                # h == w: gl_vae_decode
    new = torch.empty_like(old)
    for graph in (0, 1, 1):
        _lib.check(l.gl_vae_decode_hw(dec.handle, z.data_ptr(), 2, 8, 8, new.data_ptr(), graph, st), "gl_vae_decode_hw")
        assert torch.equal(new, old)
    enc = dec.encoder
    x = T(np.clip(recipe.normal("rect.sq.x", (2, 3, 16, 16), 3) * np.float32(0.5), -1, 1)).to(DEV)
    noise = T(recipe.normal("rect.sq.n", (2, 4, 8, 8), 3)).to(DEV)
    zo = enc.encode(x, noise)                                          # gl_vae_encode
    zn = torch.empty_like(zo)
    for graph in (0, 1, 1):
        _lib.check(l.gl_vae_encode_hw(enc.handle, x.data_ptr(), 2, 16, 16, noise.data_ptr(), zn.data_ptr(), graph, st), "gl_vae_encode_hw")
        assert torch.equal(zn, zo)
    assert torch.equal(dec.decode(z), old) and torch.equal(enc.encode(x, noise), zo)
    # shape rules of the encoder entry, per axis
    for bad in ((16, 13), (13, 16), (16, 1024), (0, 16)):
        assert l.gl_vae_encode_hw(enc.handle, x.data_ptr(), 2, bad[0], bad[1], noise.data_ptr(), zn.data_ptr(), 0, st) == -1
    for bad in ((1, 3, 16, 13), (1, 3, 1024, 16), (1, 4, 16, 24)):
        with pytest.raises(ValueError):
            enc.encode(torch.zeros(bad))


# ------------------------------------------------------------------------------------------- 3. graphs and keys
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
def test_graph_replay_equals_eager_and_shapes_alternate_on_one_handle(strict):
    shapes = [(16, 24), (24, 16), 16]
    inps = {s: tiny_inputs(s, seed=77) for s in shapes}

    def run(eng, s, reps=1):
        set_cond(eng, inps[s], s)
        x = inps[s]["x"].to(DEV)
        return eng.forward(x, 481.0, 1.0, False, reps).clone(), eng.forward(x, 201.0, 0.0, True, reps).clone()

    # the [cond ; uncond] form with the shared prefix (reps = 2)
    z = torch.zeros_like
    cat = lambda a, b: torch.cat([a, b], 0)
    two = {}
    for s in shapes:
        i = inps[s]
        two[s] = dict(context=cat(i["context"], i["uc"]), relations=cat(i["relations"], i["relations"]), boxes=cat(i["boxes"], z(i["boxes"])),
                      masks=cat(i["masks"], z(i["masks"])), positive_embeddings=cat(i["positive_embeddings"], z(i["positive_embeddings"])))

    def run2(eng, s):
        set_cond(eng, two[s], s)
        return eng.forward(inps[s]["x"].to(DEV), 481.0, 1.0, False, 2).clone()

    # fresh engine per shape, eager: the reference results
    fresh, fresh2 = {}, {}
    for s in shapes:
        import dataclasses
        cfg = dataclasses.replace(TINY, split_weights=True) if strict else TINY
        m = UNetModel(cfg, recipe.state_dict(TINY, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(TINY, 0))
        if strict:
            m.set_strict(True)
        m.engine.use_graphs = False
        fresh[s] = run(m.engine, s)
        m.engine.use_graphs = True
        again = run(m.engine, s), run(m.engine, s)                      # capture, then replay: bitwise the eager result
        for got in again:
            assert torch.equal(got[0], fresh[s][0]) and torch.equal(got[1], fresh[s][1]), s
        m.engine.use_graphs = False
        fresh2[s] = run2(m.engine, s)
        assert torch.isfinite(fresh2[s]).all() and tuple(fresh2[s].shape[-2:]) == tuple(fresh[s][0].shape[-2:])
        del m
    assert tuple(fresh[(16, 24)][0].shape) == (2, 4, 16, 24) and tuple(fresh[(24, 16)][0].shape) == (2, 4, 24, 16)
    # one engine, shapes alternating (pool tags and graph keys must not collide): every visit reproduces the fresh result
    eng = tiny_model(strict).engine
    for s in shapes + shapes[::-1] + shapes:
        got = run(eng, s)
        assert torch.equal(got[0], fresh[s][0]) and torch.equal(got[1], fresh[s][1]), s
    # the same for the 2B form: graph capture and replay on the shared engine, shapes alternating, against the fresh eager result
    for s in shapes + shapes:
        assert torch.equal(run2(eng, s), fresh2[s]), s


def test_vae_rect_engine_equals_op_sequence_and_keys_do_not_collide():
    dec = VAEDecoder(tgi.enc_sd(VAE_TINY), VAE_TINY, DEV)
    zs = {s: T(recipe.normal(f"rect.vz.{s}", (2, 4) + s, 3)) * np.float32(0.18215) for s in ((8, 12), (12, 8), (8, 8))}
    ref = {s: dec.decode_oplevel(z) for s, z in zs.items()}
    dec.use_graphs = False
    for s, z in zs.items():
        assert torch.equal(dec.decode(z), ref[s])
    dec.use_graphs = True
    for s in list(zs) * 3:
        out = dec.decode(zs[s])
        assert tuple(out.shape) == (2, 3, 2 * s[0], 2 * s[1]) and torch.equal(out, ref[s]), s
    enc = dec.encoder
    xs = {s: T(np.clip(recipe.normal(f"rect.vx.{s}", (2, 3) + s, 3) * np.float32(0.5), -1, 1)) for s in ((32, 48), (48, 32), (32, 32))}
    ns = {s: T(recipe.normal(f"rect.vn.{s}", (2, 4, s[0] // 2, s[1] // 2), 3)) for s in xs}
    eref = {s: enc.encode_oplevel(xs[s], ns[s]) for s in xs}
    enc.use_graphs = False
    for s in xs:
        assert torch.equal(enc.encode(xs[s], ns[s]), eref[s])
    enc.use_graphs = True
    for s in list(xs) * 3:
        assert torch.equal(enc.encode(xs[s], ns[s]), eref[s]), s


# ------------------------------------------------------------------------------------------- 4. full size, both modes, both orientations
@pytest.mark.parametrize("hw", [(64, 96), (96, 64)], ids=["64x96", "96x64"])
def test_default_mode_full_size_rect_at_2B8_vs_oracle(hw):
    """The config-2 UNet at 6144 / 1536 / 384 / 96 tokens per level, 2B = 8, built as test_gpu_configs builds its 64^2 / 96^2 cases: cond and
    uncond rows against the oracle, fuser on, then the scale-0 / SD-first-conv form; BOUND_FULL / FRAC_FULL of test_gpu_configs.py."""
    model, sd, fc, cfg = tgc.full_model()
    B, k = 4, 1
    inp, two = tgc.cfg_batch(cfg, B, hw, 8, seed=2024)
    assert tuple(inp["x"].shape) == (B, 4) + hw
    eng = model.engine
    eng.set_conditioning(two["context"], two["relations"], two["boxes"], two["masks"], two["positive_embeddings"], hw)
    x = inp["x"].half().float().to(DEV)
    e_on = eng.forward(x, 481.0, 1.0, False, 2).clone()
    e_off = eng.forward(x, 201.0, 0.0, True, 2).clone()
    assert tuple(e_on.shape) == (2 * B, 4) + hw
    tag = f"{hw[0]}x{hw[1]} default 2B=8"
    rows = [(f"{tag} cond  fuser on ", e_on[k:k + 1], tgc.oracle_one(sd, cfg, inp, k, True, 481)),
            (f"{tag} uncond fuser on ", e_on[B + k:B + k + 1], tgc.oracle_one(sd, cfg, inp, k, False, 481)),
            (f"{tag} cond  fuser off", e_off[k:k + 1], tgc.oracle_one(sd, cfg, inp, k, True, 201, 0.0, fc))]
    r = []
    for name, out, ref in rows:
        d = (out.float().cpu() - ref).abs()
        frac = float((d > 1e-4 + 1e-3 * ref.abs()).float().mean())
        note(f"[{name}] rel_l2={rel_l2(out, ref):.3e} outside rtol1e-3/atol1e-4: {100 * frac:.2f}% (bounds {BOUND_FULL:.1e} / {100 * FRAC_FULL:.0f}%)")
        r.append(tgc.report(name, out, ref, FRAC_FULL))
    assert max(r) < BOUND_FULL, r
    assert rel_l2(e_on[0:1], e_on[1:2]) > 1e-2 and rel_l2(e_on[0:1], e_on[B:B + 1]) > 1e-3
    assert torch.equal(e_on, eng.forward(x, 481.0, 1.0, False, 2))


@pytest.mark.parametrize("hw", [(64, 96), (96, 64)], ids=["64x96", "96x64"])
def test_strict_mode_full_size_rect_at_2B8_vs_oracle(hw):
    """Strict mode on the split weight layout (unrounded fp32 weights, fp32 latent and context): at most 0.1 % of the elements outside
    rtol 1e-3 / atol 1e-4 and rel-L2 < 3e-5, the contract of test_gpu_configs.test_strict_mode_meets_north_star_tolerance_at_bench_batch."""
    m, sd_cpu, fc_cpu, cfg = tgc.strict_model()
    eng = m.engine
    eng.clear_options()
    eng.set_option(50, 1)
    try:
        B, k = 4, 1
        inp, two = tgc.cfg_batch(cfg, B, hw, 8, seed=2024)
        eng.set_conditioning(two["context"], two["relations"], two["boxes"], two["masks"], two["positive_embeddings"], hw)
        x = inp["x"].to(DEV)
        e = eng.forward(x, 481.0, 1.0, False, 2).clone()
        e_off = eng.forward(x, 201.0, 0.0, True, 2).clone()
        tag = f"{hw[0]}x{hw[1]} STRICT 2B=8"
        rows = [(f"{tag} cond  fuser on ", e[k:k + 1], tgc.oracle_one(sd_cpu, cfg, inp, k, True, 481, round_x=False, round_ctx=False)),
                (f"{tag} uncond fuser on ", e[B + k:B + k + 1], tgc.oracle_one(sd_cpu, cfg, inp, k, False, 481, round_x=False, round_ctx=False)),
                (f"{tag} cond  fuser off", e_off[k:k + 1], tgc.oracle_one(sd_cpu, cfg, inp, k, True, 201, 0.0, fc_cpu, round_x=False, round_ctx=False))]
        r = []
        for name, out, ref in rows:
            d = (out.float().cpu() - ref).abs()
            frac = float((d > 1e-4 + 1e-3 * ref.abs()).float().mean())
            note(f"[{name}] rel_l2={rel_l2(out, ref):.3e} outside rtol1e-3/atol1e-4: {100 * frac:.4f}% (bounds {STRICT_L2:.0e} / 0.1%)")
            r.append(tgc.report(name, out, ref, STRICT_FRAC))
        assert max(r) < STRICT_L2, r
        assert torch.equal(e, eng.forward(x, 481.0, 1.0, False, 2))
    finally:
        eng.clear_options()


# ------------------------------------------------------------------------------------------- 5. full-size VAE
def _vae_oracle_sd(sd, fp32_key):
    osd = {k: (T(np.asarray(v)).half().float() if np.asarray(v).ndim >= 2 else T(np.asarray(v))) for k, v in sd.items()}
    osd[fp32_key] = T(np.asarray(sd[fp32_key]))          # applied in fp32 by the engine
    return osd


def test_vae_full_size_rect_decode_vs_oracle():
    """test_gpu_vae.test_vae_full_size_vs_oracle at [2, 4, 64, 96] -> [2, 3, 512, 768] (mid attention over 6144 tokens)."""
    cfg = VAEConfig()
    sd = recipe.vae_state_dict(cfg, 0)
    z = T(recipe.normal("rect.vae.zfull", (2, 4, 64, 96), 9)) * np.float32(0.18215 * 1.5)
    dec = VAEDecoder(sd, cfg, DEV)
    out = dec.decode(z)
    assert tuple(out.shape) == (2, 3, 512, 768)
    with torch.no_grad():
        torch.set_num_threads(min(os.cpu_count() or 1, 32))
        ref = vae_ref.decode(_vae_oracle_sd(sd, "post_quant_conv.weight"), z, cfg.ch_mult, cfg.num_res_blocks, cfg.scale_factor)
    r = rel_l2(out, ref)
    note(f"[vae_full 64x96] decode rel_l2={r:.3e} max|err|={float((out.cpu() - ref).abs().max()):.3e}")
    assert torch.isfinite(out).all() and r < VAE_BOUND, r
    assert torch.equal(out, dec.decode(z))


def test_vae_full_size_rect_encode_vs_fp32_mirror():
    """test_gpu_inpaint.test_full_size_encoder_vs_fp32_mirror at [1, 3, 512, 768] -> [1, 4, 64, 96]."""
    cfg = VAEConfig()
    sd = tgi.enc_sd(cfg)
    x = T(np.clip(recipe.normal("rect.encfull.x", (1, 3, 512, 768), 9) * np.float32(0.5), -1, 1))
    noise = T(recipe.normal("rect.encfull.n", (1, 4, 64, 96), 9))
    enc = VAEEncoder(sd, cfg, DEV)
    z = enc.encode(x, noise)
    with torch.no_grad():
        torch.set_num_threads(16)
        ref, _ = vae_encoder_pyref.encode(_vae_oracle_sd(sd, "quant_conv.weight"), x, cfg.ch_mult, cfg.num_res_blocks, noise, cfg.scale_factor)
    r = rel_l2(z, ref)
    note(f"[vae_enc_full 512x768] rel_l2={r:.3e} max|err|={float((z.cpu() - ref).abs().max()):.3e}")
    assert tuple(z.shape) == (1, 4, 64, 96) and torch.isfinite(z).all() and r < VAE_BOUND, r
    assert torch.equal(z, enc.encode(x, noise))


# ------------------------------------------------------------------------------------------- 6. conv forms at non-square maps
# (the audit changed no kernel: these pin the forms whose addressing depends on the row length W -- halo, stride 2, nearest 2x, the
# encoder's pad-(0,1) window -- at W != H, W not a power of two, and the power-of-two-W / non-power-of-two-HW mix, on the 4-wave and the
# 8-wave kernels; fp16-representable operands against torch fp32 on the CPU, the bound of test_conv3x3_pad01_matches_padded_conv)
CONV_RECT = [(2, 64, 64, 8, 12), (2, 64, 128, 12, 8), (1, 320, 320, 64, 96), (1, 320, 320, 96, 64), (2, 128, 64, 16, 24), (8, 640, 640, 12, 8)]


@pytest.mark.parametrize("form", ["same", "stride2", "up2x", "pad01"])
@pytest.mark.parametrize("B,Cin,Cout,h,w", CONV_RECT)
def test_conv_forms_at_rect_maps(B, Cin, Cout, h, w, form):
    init_device()
    x = T(recipe.normal(f"rect.conv.x.{Cin}.{h}.{w}", (B, Cin, h, w), 3)).half().float()
    wt = (T(recipe.normal(f"rect.conv.w.{Cin}.{Cout}", (Cout, Cin, 3, 3), 3)) * np.float32((9 * Cin) ** -0.5)).half().float()
    b = T(recipe.normal(f"rect.conv.b.{Cout}", (Cout,), 3))
    with torch.no_grad():
        torch.set_num_threads(16)
        if form == "same":
            ref = F.conv2d(x, wt, b, padding=1)
        elif form == "stride2":
            ref = F.conv2d(x, wt, b, stride=2, padding=1)
        elif form == "up2x":
            ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, b, padding=1)
        else:
            ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)
    xd = x.permute(0, 2, 3, 1).reshape(B * h * w, Cin).half().to(DEV).contiguous()
    kw = {"same": {}, "stride2": dict(stride=2), "up2x": dict(upsample2x=True), "pad01": dict(pad01=True)}[form]
    _conv_vs_ref(xd, wt, b, B, h, w, ref, f"conv {form} B={B} {Cin}->{Cout}", **kw)


# ------------------------------------------------------------------------------------------- 7. boundary
@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt_rect")
    p = str(d / "tiny_gligen_rect.pth")
    ck = stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)
    ck["autoencoder"].update({k: T(np.asarray(v)) for k, v in recipe.vae_encoder_state_dict(VAE_TINY, 0).items()})
    torch.save(ck, p)
    stubs.install_fake_sng_parser()
    am = itf.load_all_models(p, DEV)
    return p, am, stubs.toy_clip().to(DEV), stubs.ToyProcessor()


LOC = [[0.10, 0.10, 0.50, 0.55], [0.55, 0.20, 0.90, 0.70]]


@pytest.mark.parametrize("hw", [(16, 24), (24, 16)], ids=["16x24", "24x16"])
def test_run_one_image_with_rect_noise_returns_rect_images(loaded, hw):
    p, am, clip, proc = loaded
    am[0].first_conv_type = "GLIGEN"
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5])
    torch.manual_seed(5)
    noise = torch.randn(1, 4, *hw).to(DEV)
    imgs = itf.run_one_image(am, dict(batch_size=1, no_plms=False, guidance_scale=7.5, steps=4), meta, noise, clip, proc, device=DEV)
    f = 2                                                  # VAE_TINY's factor
    assert len(imgs) == 1 and imgs[0].size == (f * hw[1], f * hw[0]) and imgs[0].mode == "RGB"      # PIL size is (width, height)
    a = np.asarray(imgs[0])
    assert a.shape == (f * hw[0], f * hw[1], 3) and a.std() > 0


def test_generate_batch_images_sized_on_the_stubbed_towers(loaded):
    p, am, clip, proc = loaded
    am[0].first_conv_type = "GLIGEN"
    seen = {}
    orig = itf.run_batch_images

    def spy(all_models, args, meta, starting_noise, *a, **k):
        seen["noise"] = tuple(starting_noise.shape)
        return orig(all_models, dict(args, steps=4), meta, starting_noise, *a, **k)
    itf.run_batch_images = spy
    try:
        imgs = itf.generate_batch_images_sized(am, ["cat sitting on mat", "a quiet street"], [["cat"], ["street"]],
                                               [[[0.1, 0.1, 0.5, 0.5]], [[0.0, 0.5, 1.0, 1.0]]], clip, proc, device=DEV, height=32, width=48)
    finally:
        itf.run_batch_images = orig
    assert seen["noise"] == (2, 4, 16, 24)
    assert len(imgs) == 2 and all(im.size == (48, 32) for im in imgs)
    with pytest.raises(ValueError):
        itf.generate_batch_images_sized(am, ["a"], [["a"]], [[[0.1, 0.1, 0.5, 0.5]]], clip, proc, device=DEV, height=40, width=48)


def test_inpainting_a_non_square_image_keeps_the_known_region(loaded):
    p, am, clip, proc = loaded
    model, autoencoder = am[0], am[1]
    img = tgi._input_image()                                # 56 x 40 pixels, resized to (W, H) = (48, 32)
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5], input_image=img)
    seen = {}
    orig = itf.denoise

    def spy(*a, **k):
        seen["k"] = k
        seen["lat"] = orig(*a, **k)
        return seen["lat"]
    itf.denoise = spy
    try:
        model.first_conv_type = "GLIGEN"
        torch.manual_seed(21)
        imgs = itf.run_one_image(am, dict(batch_size=2, no_plms=False, guidance_scale=7.5, steps=4), meta, torch.randn(2, 4, 16, 24).to(DEV), clip, proc,
                                 device=DEV)
    finally:
        itf.denoise = orig
    mask, z0, lat = seen["k"]["mask"], seen["k"]["x0"], seen["lat"]
    assert tuple(mask.shape) == (2, 1, 16, 24) and tuple(z0.shape) == (1, 4, 16, 24) and tuple(lat.shape) == (2, 4, 16, 24)
    torch.manual_seed(21)                                   # the posterior sample draws from the CPU generator right after the starting noise
    torch.randn(2, 4, 16, 24)
    assert torch.equal(z0, autoencoder.encode(itf.load_input_image(img, (32, 48), DEV)))
    boxes = np.zeros((2, 30, 4), np.float32)
    boxes[:, :2] = np.asarray(LOC, np.float32)
    assert np.array_equal(mask.cpu().numpy(), rc.rect_mask_rule(boxes, 16, 24))
    # test_gpu_inpaint.test_run_one_image_inpaints_like_the_manual_chain's bound: outside the boxes the final latent stays closer to x0
    keep = mask.bool().expand_as(lat)
    dlt = (lat - z0.expand_as(lat)).abs()
    assert float(dlt[keep].mean()) < float(dlt[~keep].mean())
    assert len(imgs) == 2 and imgs[0].size == (48, 32)


def test_bad_latent_shapes_raise_before_anything_is_launched(loaded):
    p, am, clip, proc = loaded
    model = am[0]
    eng = model.engine
    meta = dict(prompt="cat sitting on mat", phrases=["cat", "mat"], locations=LOC, alpha_type=[0.5, 0.0, 0.5])
    args = dict(batch_size=1, no_plms=False, guidance_scale=7.5, steps=2)
    set_cond(eng, tiny_inputs(16), 16)
    before = dict(eng.cond)
    with pytest.raises(ValueError, match="multiple of 8"):
        itf.run_one_image(am, args, meta, torch.randn(1, 4, 12, 20).to(DEV), clip, proc, device=DEV)
    assert eng.cond == before                               # rejected on the host: the conditioning was not replaced, nothing ran
    # a latent whose shape disagrees with the conditioning: both transposed and truncated forms (they used to be read as 16 x 16)
    set_cond(eng, tiny_inputs((16, 24)), (16, 24))
    for bad in ((2, 4, 24, 16), (2, 4, 16, 16), (2, 4, 24, 24), (2, 4, 8, 24)):
        with pytest.raises(ValueError, match="does not match"):
            eng.forward(torch.zeros(bad, device=DEV), 481.0, 1.0, False, 1)
    set_cond(eng, tiny_inputs(16), 16)
    for bad in ((2, 4, 24, 16), (2, 4, 16, 24)):            # [.., 24, 16] passed the old last-axis-only check
        with pytest.raises(ValueError, match="does not match"):
            eng.forward(torch.zeros(bad, device=DEV), 481.0, 1.0, False, 1)
    assert torch.isfinite(eng.forward(tiny_inputs(16)["x"].to(DEV), 481.0, 1.0, False, 1)).all()
