"""VAE decode stage on a real MI355X: HIP path vs the reference golden (tiny config) and vs the
pinned oracle live on the host CPU (full-size decoder, 64x64 latent -> 512x512 image)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import golden_cases as gc
from layoutllm_t2i_amd import ops, recipe
from layoutllm_t2i_amd._lib import init_device
from layoutllm_t2i_amd.arch import VAE_TINY, VAEConfig
from layoutllm_t2i_amd.vae import VAEDecoder
from oracle import vae_ref

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_softmax_rows_and_latent_pack():
    init_device()
    x = T(recipe.normal("vae.sm", (300, 4096), 5)) * 3
    xd = x.to(torch.float16).to(DEV)
    xr = xd.float().cpu()
    ops.softmax_rows(xd, 0.7)
    ref = F.softmax(xr * 0.7, dim=-1)
    assert torch.allclose(xd.float().cpu(), ref, rtol=2e-3, atol=1e-6), float((xd.float().cpu() - ref).abs().max())
    big = torch.zeros(64, 128, dtype=torch.float16, device=DEV)      # strided view: 64 valid columns of 128
    big[:, :64] = T(recipe.normal("vae.sm2", (64, 64), 5)).to(torch.float16).to(DEV)
    r2 = F.softmax(big[:, :64].float().cpu(), dim=-1)
    ops.softmax_rows(big[:, :64], 1.0)
    assert torch.allclose(big[:, :64].float().cpu(), r2, rtol=2e-3, atol=1e-6) and float(big[:, 64:].abs().max()) == 0
    z = T(recipe.normal("vae.z", (2, 4, 8, 8), 5))
    w, b = T(recipe.normal("vae.pw", (4, 4), 5)), T(recipe.normal("vae.pb", (4,), 5))
    out = torch.empty(2 * 64, 64, dtype=torch.float16, device=DEV)
    ops.latent_affine_pack(z.to(DEV), w.to(DEV), b.to(DEV), 1 / 0.18215, 64, out)
    ref = F.conv2d(z / 0.18215, w.view(4, 4, 1, 1), b).permute(0, 2, 3, 1).reshape(128, 4)
    assert torch.allclose(out[:, :4].float().cpu(), ref, rtol=1e-3, atol=1e-3) and float(out[:, 4:].abs().max()) == 0


def test_vae_tiny_matches_reference_golden():
    case = next(c for c in gc.CASES if c["name"] == "vae_tiny")
    z = T(gc.case_inputs(case)["z"])
    dec = VAEDecoder(recipe.vae_state_dict(VAE_TINY, 0), VAE_TINY, DEV)
    out = dec.decode(z)
    ref = T(np.load(os.path.join(GOLD, "vae_tiny.npz"))["out"])
    assert out.shape == ref.shape and out.dtype == torch.float32
    r = rel_l2(out, ref)
    print(f"[vae_tiny] rel_l2={r:.3e} max|err|={float((out.cpu() - ref).abs().max()):.3e} |ref|max={float(ref.abs().max()):.3f}")
    assert torch.isfinite(out).all() and r < 6e-3, r


def test_vae_full_size_vs_oracle():
    """the real decoder (49.5 M params, mid attention over 4096 tokens with d = 512, 512x512 output)"""
    cfg = VAEConfig()
    sd = recipe.vae_state_dict(cfg, 0)
    z = T(recipe.normal("vae.zfull", (1, 4, 64, 64), 9)) * np.float32(0.18215 * 1.5)
    dec = VAEDecoder(sd, cfg, DEV)
    out = dec.decode(z)
    assert out.shape == (1, 3, 512, 512)
    osd = {k: (T(np.asarray(v)).half().float() if np.asarray(v).ndim >= 2 else T(np.asarray(v))) for k, v in sd.items()}
    osd["post_quant_conv.weight"] = T(np.asarray(sd["post_quant_conv.weight"]))     # applied in fp32 by the engine
    with torch.no_grad():
        torch.set_num_threads(min(os.cpu_count() or 1, 32))
        ref = vae_ref.decode(osd, z, cfg.ch_mult, cfg.num_res_blocks, cfg.scale_factor)
    r = rel_l2(out, ref)
    print(f"[vae_full] rel_l2={r:.3e} max|err|={float((out.cpu() - ref).abs().max()):.3e} |ref|max={float(ref.abs().max()):.3f}")
    assert torch.isfinite(out).all() and r < 6e-3, r
    # decode twice: deterministic
    assert torch.equal(out, dec.decode(z))


@pytest.mark.parametrize("cfgname,B,side", [("tiny", 2, 16), ("tiny", 3, 8), ("full", 2, 32)])
def test_c_engine_equals_python_op_sequence_bitwise(cfgname, B, side):
    """gl_vae_decode (C++ plan + pool + hipGraph, csrc/vae_engine.hip) against the same launch sequence issued op by op from
    Python (VAEDecoder.decode_oplevel): eager, captured and replayed, several (batch, side) keys on one handle."""
    cfg = VAE_TINY if cfgname == "tiny" else VAEConfig()
    dec = VAEDecoder(recipe.vae_state_dict(cfg, 0), cfg, DEV)
    z = T(recipe.normal(f"vae.zc.{B}.{side}", (B, cfg.z_channels, side, side), 3)) * np.float32(0.18215)
    ref = dec.decode_oplevel(z)
    dec.use_graphs = False
    eager = dec.decode(z)
    dec.use_graphs = True
    first = dec.decode(z)                      # warm-up + capture
    replay = dec.decode(z)                     # graph replay
    assert torch.isfinite(ref).all()
    assert torch.equal(eager, ref) and torch.equal(first, ref) and torch.equal(replay, ref)
    z2 = z[:1].contiguous()                    # another key on the same handle, then back
    assert torch.equal(dec.decode(z2), dec.decode_oplevel(z2))
    assert torch.equal(dec.decode(z), ref)
    from layoutllm_t2i_amd import _lib
    assert _lib.lib().gl_vae_num_launches(dec.handle) > 20 and _lib.lib().gl_vae_pool_bytes(dec.handle) > 0


def test_graphs_survive_a_growing_pool():
    """small key first: (B = 1, side 8) captured and replayed, then (B = 2, side 16) grows pooled buffers (the earlier graph holds freed
    addresses and must be dropped), then the small key again -- every result equal to the op-by-op sequence; the encoder likewise"""
    cfg = VAE_TINY
    sd = {**recipe.vae_state_dict(cfg, 0), **recipe.vae_encoder_state_dict(cfg, 0)}
    dec = VAEDecoder(sd, cfg, DEV)
    zs = {(B, side): T(recipe.normal(f"vae.zg.{B}.{side}", (B, cfg.z_channels, side, side), 3)) * np.float32(0.18215) for B, side in ((1, 8), (2, 16))}
    refs = {k: dec.decode_oplevel(z).clone() for k, z in zs.items()}
    assert all(torch.isfinite(r).all() for r in refs.values())
    for k in ((1, 8), (1, 8), (2, 16), (1, 8)):
        assert torch.equal(dec.decode(zs[k]), refs[k]), k
    enc = dec.encoder
    f = 2 ** (len(cfg.ch_mult) - 1)
    xs = {(B, side): (T(np.clip(recipe.normal(f"vae.xg.{B}.{side}", (B, 3, side, side), 3) * np.float32(0.5), -1, 1)),
                      T(recipe.normal(f"vae.ng.{B}.{side}", (B, cfg.embed_dim, side // f, side // f), 3))) for B, side in ((1, 32), (2, 64))}
    erefs = {k: enc.encode_oplevel(x, n).clone() for k, (x, n) in xs.items()}
    assert all(torch.isfinite(r).all() for r in erefs.values())
    for k in ((1, 32), (1, 32), (2, 64), (1, 32)):
        assert torch.equal(enc.encode(*xs[k]), erefs[k]), k


def test_vae_set_option_is_per_decoder():
    """VAEDecoder.set_option (gl_vae_set_option; ADVICE r3: the method used to raise NameError): knobs set on ONE decoder (13 = 0:
    no intra-block K-split conv variants, 30 = 0: no 8-wave kernel -- other fp32 summation orders) leave its result within
    rounding of the default path, a second decoder built from the same weights is untouched, an unknown key is refused."""
    cfg = VAE_TINY
    a = VAEDecoder(recipe.vae_state_dict(cfg, 0), cfg, DEV)
    b = VAEDecoder(recipe.vae_state_dict(cfg, 0), cfg, DEV)
    z = T(recipe.normal("vae.zopt", (2, cfg.z_channels, 16, 16), 3)) * np.float32(0.18215)
    base = a.decode(z).clone()
    a.set_option(13, 0)
    a.set_option(30, 0)
    alt = a.decode(z).clone()
    assert torch.isfinite(alt).all() and rel_l2(alt, base) < 2e-3
    assert torch.equal(a.decode(z), alt)                       # replay of the graph captured under the overrides
    assert torch.equal(b.decode(z), base)
    with pytest.raises(Exception):
        a.set_option(99, 1)
