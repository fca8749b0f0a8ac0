"""Host side of grounded inpainting (no GPU): the VAE encoder's parameter list and engine weight table, the box masks, the
q_sample schedule buffers and the fp32 encoder mirror, each against the reference's own outputs (tools/make_inpaint_goldens.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import vae_encoder_pyref
from layoutllm_t2i_amd import _lib, host, recipe
from layoutllm_t2i_amd.arch import VAE_TINY, VAEConfig, vae_decoder_param_shapes, vae_encoder_param_shapes
from layoutllm_t2i_amd.model import LatentDiffusion
from layoutllm_t2i_amd.sampler import PLMSSampler
from layoutllm_t2i_amd.vae import encoder_unsupported, packed_shapes

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


@pytest.mark.parametrize("tag,cfg", [("full", VAEConfig()), ("tiny", VAE_TINY)])
def test_encoder_param_names_and_shapes_match_reference(tag, cfg):
    g = gold("vae_enc_names")
    ref = {str(n): tuple(int(d) for d in s if d) for n, s in zip(g[f"{tag}_names"], g[f"{tag}_shapes"])}
    assert vae_encoder_param_shapes(cfg) == ref


@pytest.mark.parametrize("cfg", [VAEConfig(), VAE_TINY], ids=["full", "tiny"])
def test_encoder_weight_table_covers_the_packed_tensors(cfg):
    """gl_vae_encoder_create's flat table = the packer's entries (packed_shapes, shared with VAEEncoder), 256-byte aligned,
    non-overlapping; the decoder handle's table is still exactly the decoder's."""
    for encoder, shapes in ((True, vae_encoder_param_shapes(cfg)), (False, vae_decoder_param_shapes(cfg))):
        h = _lib.create_vae(cfg, encoder=encoder)
        try:
            table, total = _lib.vae_weight_table(h)
        finally:
            _lib.lib().gl_vae_destroy(h)
        want = packed_shapes(shapes)
        assert [n for n, *_ in table] == list(dict.fromkeys(n for n, *_ in table))        # no duplicates
        assert {n for n, *_ in table} == set(want)
        end = 0
        for name, off, nbytes, dtype, shape in sorted(table, key=lambda r: r[1]):
            wshape, wdtype = want[name]
            assert shape == wshape and dtype == (0 if wdtype == torch.float16 else 1), name
            assert nbytes == int(np.prod(shape)) * (2 if dtype == 0 else 4)
            assert off % 256 == 0 and off >= end, name
            end = off + nbytes
        assert total >= end
    if cfg == VAEConfig():
        enc = packed_shapes(vae_encoder_param_shapes(cfg))
        assert enc["encoder.conv_in.w"] == ((128, 9 * 64), torch.float16)               # 3 image channels padded to 64
        assert enc["quant_conv.w"] == ((8, 8), torch.float32)


def test_encoder_create_rejects_bad_configs():
    import ctypes as C
    cc = _lib.VaeConfigC()
    cc.ch, cc.n_mult, cc.num_res_blocks, cc.z_channels, cc.out_ch, cc.embed_dim, cc.scale_factor = 128, 4, 2, 4, 3, 4, 0.18215
    for i, m in enumerate((1, 2, 4, 4)):
        cc.ch_mult[i] = m
    h = C.c_void_p()
    assert _lib.lib().gl_vae_encoder_create(C.byref(cc), C.byref(h)) == 0
    _lib.lib().gl_vae_destroy(h)
    for field, bad in (("out_ch", 65), ("embed_dim", 0), ("ch", 96)):
        c2 = _lib.VaeConfigC.from_buffer_copy(cc)
        setattr(c2, field, bad)
        assert _lib.lib().gl_vae_encoder_create(C.byref(c2), C.byref(h)) == -1, field        # GL_ERR_BAD_ARG


def test_unsupported_encoders_are_named():
    cfg = VAEConfig()
    sd = {k: np.zeros(s, np.float32) for k, s in vae_encoder_param_shapes(cfg).items()}
    assert encoder_unsupported(sd, cfg) is None
    assert "attention" in encoder_unsupported({**sd, "encoder.down.3.attn.0.q.weight": np.zeros((1,))}, cfg)
    sd4 = dict(sd)
    sd4["encoder.conv_in.weight"] = np.zeros((128, 4, 3, 3), np.float32)
    assert "input channels" in encoder_unsupported(sd4, cfg)


@pytest.mark.parametrize("size", [64, 16, 13])
def test_draw_masks_from_boxes_matches_reference(size):
    g = gold("inpaint_masks")
    got = host.draw_masks_from_boxes(T(g["boxes"]), size)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), g[f"mask_{size}"])
    assert np.array_equal(host.draw_masks_from_boxes(g["boxes"], size).numpy(), g[f"mask_{size}"])   # numpy boxes too


def test_q_sample_schedule_buffers_match_reference():
    g = gold("inpaint_schedule")
    d = LatentDiffusion(device="cpu")
    assert d.sqrt_alphas_cumprod.dtype == torch.float32
    assert np.array_equal(d.sqrt_alphas_cumprod.numpy(), g["sqrt_alphas_cumprod"])
    assert np.array_equal(d.sqrt_one_minus_alphas_cumprod.numpy(), g["sqrt_one_minus_alphas_cumprod"])
    # q_sample = extract_into_tensor(buffers, t) (ldm.py:19-22), broadcasting a batch-1 x0 over the t batch
    x0 = T(recipe.normal("inpaint.qs.x0", (1, 4, 8, 8), 3))
    n = T(recipe.normal("inpaint.qs.n", (1, 4, 8, 8), 3))
    t = torch.tensor([981, 981])
    a = T(g["sqrt_alphas_cumprod"])[t].reshape(2, 1, 1, 1)
    s = T(g["sqrt_one_minus_alphas_cumprod"])[t].reshape(2, 1, 1, 1)
    assert torch.equal(d.q_sample(x0, t, n), a * x0 + s * n)


def test_mask_without_x0_fails_like_the_reference():
    class _M:
        device = torch.device("cpu")
    s = PLMSSampler(LatentDiffusion(device="cpu"), _M())
    with pytest.raises(AssertionError):
        s.plms_sampling((1, 4, 8, 8), dict(x=torch.zeros(1, 4, 8, 8)), mask=torch.ones(1, 1, 8, 8), x0=None)


def test_fp32_encoder_mirror_matches_reference_golden():
    g = gold("vae_enc_tiny")
    cfg = VAE_TINY
    sd = {k: T(np.asarray(v)) for k, v in {**recipe.vae_state_dict(cfg, 0), **recipe.vae_encoder_state_dict(cfg, 0)}.items()}
    with torch.no_grad():
        z, mean = vae_encoder_pyref.encode(sd, T(g["x"]), cfg.ch_mult, cfg.num_res_blocks, T(g["noise"]), cfg.scale_factor)
    for got, name in ((mean, "mean"), (z, "z")):
        ref = T(g[name])
        r = float((got - ref).norm() / ref.norm())
        assert got.shape == ref.shape and r < 1e-6, (name, r)
    # the recorded noise is what torch.manual_seed(seed); torch.randn(mean.shape) draws on the CPU (distributions.py:36)
    torch.manual_seed(int(g["seed"]))
    assert torch.equal(torch.randn(tuple(mean.shape)), T(g["noise"]))
