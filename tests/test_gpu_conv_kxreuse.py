"""The kx-reuse main loop of the 8-wave 3x3 conv (csrc/gemm8.hip KXR, gl_set_option key 54) against the plain loop, torch and shifted copies.

Every launch goes through ops.conv3x3 with the 8-wave kernel forced (key 30 = 2), 256-row tiles (key 46 = 0) and the split-K plan pinned by
key 34 (the minimum K-tiles per slice: 1000 = no split).  The new loop issues the same MFMA sequence on the same operand values as the plain
loop, so old == new is asserted bitwise; gl_debug_read(11) counts the launches the kx-reuse loop served, so a dispatcher that quietly kept the
plain loop (or took the new one for an ineligible launch) cannot pass."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from layoutllm_t2i_amd import ops, recipe
from layoutllm_t2i_amd._lib import EPI_BIAS, EPI_RES, init_device
from layoutllm_t2i_amd.weights import pack_conv3x3

DEV = "cuda:0"
RTOL, ATOL = 1e-3, 1e-4            # the conv cases of tests/test_gpu_kernels.py: |err| <= ATOL * max(1, max|ref|) + RTOL * |ref|, no outliers
DEFAULTS = {30: 1, 34: 11, 46: 11, 54: 2}


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()
    yield
    _opts(DEFAULTS)


def _opts(d):
    for k, v in d.items():
        ops.set_option(k, v)


def _force(kxr, minkt=1000):
    _opts({30: 2, 46: 0, 34: minkt, 54: kxr})


def _nhwc(x):  # [B,C,H,W] -> [B*H*W, C]
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


_cases = {}


def _case(B, H, W, Cin, Cout):
    """fp16-rounded operands (CPU fp32 and device fp16) and the fp32 torch reference, computed once per shape and left unchanged"""
    key = (B, H, W, Cin, Cout)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * Cin + 10 * H + B)
        x = torch.randn(B, Cin, H, W, generator=g).half().float()
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).half().float()
        b = torch.randn(Cout, generator=g) * 0.1
        res = torch.randn(B * H * W, Cout, generator=g)
        _cases[key] = dict(x=x, w=w, b=b, res=res, xd=_nhwc(x).half().to(DEV), wd=pack_conv3x3(w).to(DEV), bd=b.to(DEV), resd=res.to(DEV),
                           ref=_nhwc(F.conv2d(x, w, b, padding=1)))
    return _cases[key]


def _run(c, B, H, W, f32res=False, stride=1, up=False):
    """one launch into poisoned outputs; returns the outputs and how many launches the 8-wave kernel / its kx-reuse loop served"""
    Cout = c["wd"].shape[0]
    ho, wo = (2 * H, 2 * W) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    M = B * ho * wo
    n8, nx = ops.gemm8_launch_count(), ops.kxreuse_launch_count()
    if f32res:
        out = torch.full((M, Cout), 7.0, dtype=torch.float32, device=DEV)
        o16 = torch.full((M, Cout), 7.0, dtype=torch.float16, device=DEV)
        ops.conv3x3(c["xd"], c["wd"], out, B, H, W, c["bd"], epi=EPI_RES, res=c["resd"][:M], out16=o16, stride=stride, upsample2x=up)
        outs = (out, o16)
    else:
        out = torch.full((M, Cout), 7.0, dtype=torch.float16, device=DEV)
        ops.conv3x3(c["xd"], c["wd"], out, B, H, W, c["bd"], epi=EPI_BIAS, stride=stride, upsample2x=up)
        outs = (out,)
    torch.cuda.synchronize()
    return outs, ops.gemm8_launch_count() - n8, ops.kxreuse_launch_count() - nx


def _old_new(c, B, H, W, minkt=1000, **kw):
    _force(0, minkt)
    old, n8, nx = _run(c, B, H, W, **kw)
    assert (n8, nx) == (1, 0), ("key 54 = 0 must run the plain loop of the 8-wave kernel", n8, nx)
    _force(1, minkt)
    new, n8, nx = _run(c, B, H, W, **kw)
    assert n8 == 1, n8
    return old, new, nx


# the smallest shapes that reach every mechanism: (B, H, W, Cin, Cout)
SHAPES = [
    (5, 8, 8, 64, 160),        # M = 320: second tile partial, tiles span samples, one channel block
    (2, 16, 16, 128, 128),     # 128-wide tile, two channel blocks: the A buffers swap
    (1, 24, 40, 128, 160),     # division path, image rows not aligned to tile rows
    (1, 64, 64, 64, 320),      # two N tiles, 16 M tiles, interior tiles without a vertical halo
]


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_bitwise_equal_to_plain_loop(B, H, W, Cin, Cout):
    c = _case(B, H, W, Cin, Cout)
    old, new, nx = _old_new(c, B, H, W)
    assert nx == 1, "the kx-reuse loop did not take an eligible launch"
    assert torch.equal(old[0], new[0])


def test_bitwise_equal_fp32_residual_output():
    B, H, W, Cin, Cout = SHAPES[1]
    c = _case(B, H, W, Cin, Cout)
    old, new, nx = _old_new(c, B, H, W, f32res=True)
    assert nx == 1
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])


@pytest.mark.parametrize("kper", [9, 18])
def test_bitwise_equal_split_k(kper):
    """Cin = 256: 36 K-tiles in slices of 9 and 18 (key 34 = the minimum slice length, which the two-tile grid then takes), with the reduction"""
    B, H, W, Cin, Cout = 2, 16, 16, 256, 128
    c = _case(B, H, W, Cin, Cout)
    for f32res in (False, True):
        old, new, nx = _old_new(c, B, H, W, minkt=kper, f32res=f32res)
        assert nx == 1
        for a, b in zip(old, new):
            assert torch.equal(a, b)
    ref = c["ref"] + c["res"]                                   # every slice was summed: the fp32 output against torch, same rule as below
    err = (new[0].cpu() - ref).abs()
    assert bool((err <= ATOL * max(1.0, float(ref.abs().max())) + RTOL * ref.abs()).all()), float(err.max())


def test_tap_isolation():
    """Weights = one tap (ky, kx) of an identity over channels: the output is the input shifted by that tap with exact zeros in the halo (one
    product per output: exact).  Catches a wrong shift, a missed horizontal mask at ox = 0 / Win - 1 and a read of the neighbouring sample's
    last row at oy = 0, per tap.  B = 2 (M = 128) is below the 8-wave kernel's 256-row minimum and runs wherever the dispatcher sends it; B = 5
    (M = 320: a partial second tile, tiles that span samples) is the same check on the kx-reuse loop itself."""
    H = W = 8
    C = 64
    for B in (2, 5):
        g = torch.Generator().manual_seed(77 + B)
        x = torch.randn(B, C, H, W, generator=g).half()
        xd = _nhwc(x).to(DEV)
        for ky in range(3):
            for kx in range(3):
                w = torch.zeros(C, C, 3, 3)
                w[torch.arange(C), torch.arange(C), ky, kx] = 1.0
                want = torch.zeros_like(x)
                ys, xs = slice(max(0, 1 - ky), min(H, H + 1 - ky)), slice(max(0, 1 - kx), min(W, W + 1 - kx))
                yi, xi = slice(max(0, ky - 1), min(H, H + ky - 1)), slice(max(0, kx - 1), min(W, W + kx - 1))
                want[:, :, ys, xs] = x[:, :, yi, xi]
                _force(1)
                nx = ops.kxreuse_launch_count()
                out = torch.full((B * H * W, C), 7.0, dtype=torch.float16, device=DEV)
                ops.conv3x3(xd, pack_conv3x3(w).to(DEV), out, B, H, W, None)
                torch.cuda.synchronize()
                if B == 5:
                    assert ops.kxreuse_launch_count() == nx + 1
                assert torch.equal(out.cpu(), _nhwc(want)), (B, ky, kx)


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_against_torch_fp32(B, H, W, Cin, Cout):
    c = _case(B, H, W, Cin, Cout)
    _force(1)
    (out,), _, nx = _run(c, B, H, W)
    assert nx == 1
    out, ref = out.float().cpu(), c["ref"]
    assert torch.isfinite(out).all()
    err = (out - ref).abs()
    tol = ATOL * max(1.0, float(ref.abs().max())) + RTOL * ref.abs()
    bad = float((err > tol).float().mean())
    print(f"[kxr conv {B}x{H}x{W} {Cin}->{Cout}] max|err|={float(err.max()):.3e} |ref|max={float(ref.abs().max()):.3f} viol={bad:.2e}")
    assert bad == 0.0, (bad, float(err.max()))


def test_ineligible_launches_take_the_plain_loop():
    """stride 2, nearest-2x upsample and slices of 10 K-tiles: key 54 = 1 must give the bits of key 54 = 0 through the plain loop"""
    # (B, H, W, Cin, Cout, minkt, kwargs); the last: 90 K-tiles on one tile -> 9 slices of 10
    for B, H, W, Cin, Cout, minkt, kw in [(2, 32, 32, 128, 128, 1000, dict(stride=2)), (2, 8, 8, 128, 128, 1000, dict(up=True)),
                                          (1, 16, 16, 640, 128, 10, dict())]:
        c = _case(B, H, W, Cin, Cout)
        old, new, nx = _old_new(c, B, H, W, minkt=minkt, **kw)
        assert nx == 0, ("an ineligible launch took the kx-reuse loop", kw, minkt)
        assert torch.equal(old[0], new[0])


def test_tiny_engine_forward_equal_under_both_loops():
    """one TINY-config engine forward, then the same forward in the same process with the key flipped"""
    from layoutllm_t2i_amd.arch import TINY
    from layoutllm_t2i_amd.model import GroundingNetInput, UNetModel
    T = torch.from_numpy
    m = UNetModel(TINY, recipe.state_dict(TINY, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(TINY, 0))
    m.grounding_tokenizer_input = GroundingNetInput()
    inp = {k: T(v) for k, v in recipe.synth_inputs(TINY, 2, 16, n_boxes=4, n_rel=3, seed=4321).items()}
    eng = m.engine
    eng.set_conditioning(inp["context"], inp["relations"], inp["boxes"], inp["masks"], inp["positive_embeddings"], 16)
    x = inp["x"].to(DEV)
    outs, served = [], []
    for kxr in (0, 1):
        _force(kxr)
        nx = ops.kxreuse_launch_count()
        outs.append(eng.forward(x, 981.0, 1.0, False, 1).clone())
        torch.cuda.synchronize()
        served.append(ops.kxreuse_launch_count() - nx)
    _opts(DEFAULTS)
    assert served[0] == 0 and served[1] > 0, served
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
