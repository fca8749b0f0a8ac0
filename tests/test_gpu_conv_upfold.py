"""Upsample convs as four folded 2x2 convs on the GPU (csrc/gemm8.hip UPF, gl_conv_args.upsample2x = 2, option key 55).

(a) exact cases: integer-valued x (|x| <= 4), weights in {-2..2} / 4 and biases in multiples of 1/4, so every product, every folded weight and
    every partial sum is exact in fp32 whatever the summation order -- the folded launch, the 9-tap launch and the fp64 reference must agree
    bitwise; gl_debug_read(12) must move by exactly the number of folded launches;
(b) random values against the fp64 conv of the fp16-rounded x and the UNROUNDED w, rel-L2 < 1e-3 (the bound of the project's conv tests), the
    9-tap launch printed beside it;
(c) bad arguments;
(d) the TINY engine and the small VAE decoder built under key 55 = 1 and 0 in one process, against the reference goldens."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import golden_cases as gc
from layoutllm_t2i_amd import _lib, ops, recipe
from layoutllm_t2i_amd._lib import EPI_BIAS, OUT_F16_ROWMAJOR, OUT_F32_NCHW, init_device
from layoutllm_t2i_amd.weights import pack_conv3x3, pack_conv_upfold

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
DEFAULTS = {k: _lib.lib().gl_get_option(k) for k in (34, 46, 55)}       # the process values when the module is imported, put back at the end


@pytest.fixture(scope="module", autouse=True)
def _init():
    init_device()
    yield
    for k, v in DEFAULTS.items():
        ops.set_option(k, v)


def _plan(B, H, W, Cin, Cout):
    """(tile rows, K slices) the dispatcher plans for a folded launch under the current options -- the rule of gemm_conv.hip's dispatch restated
    (key 31: split below this many tiles; key 34: minimum K-tiles per slice; key 46 bit 0 / bit 2: half-height conv tiles), so that a case
    meant for split-K or for 128-row tiles fails loudly if a later threshold change stops it from getting there"""
    get = _lib.lib().gl_get_option
    cdiv = lambda a, b: (a + b - 1) // b
    bn = 160 if Cout % 160 == 0 else 128
    nk, Ms = 4 * Cin // 64, B * H * W

    def split(tiles):
        return max(1, min(256 // tiles, nk // get(34))) if tiles < get(31) else 1
    bm, tiles = 256, 4 * cdiv(Ms, 256) * cdiv(Cout, bn)
    sk = split(tiles)
    if tiles * 2 <= 256 and ((get(46) & 4) or ((get(46) & 1) and nk // sk <= 16)):
        bm, tiles = 128, 4 * cdiv(Ms, 128) * cdiv(Cout, bn)
        sk = split(tiles)
    return bm, cdiv(nk, cdiv(nk, sk))


def _nhwc(x):  # [B,C,H,W] -> [B*H*W, C]
    B, Cc, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, Cc).contiguous()


def _ref64(x, w, b):
    return _nhwc(F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1))


_cases = {}


def _case(kind, B, H, W, Cin, Cout):
    """operands and the fp64 reference, computed once per shape and left unchanged"""
    key = (kind, B, H, W, Cin, Cout)
    if key not in _cases:
        g = torch.Generator().manual_seed(100 * Cin + 10 * H + W + B)
        if kind == "exact":
            x = torch.randint(-4, 5, (B, Cin, H, W), generator=g).float()
            w = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=g).float() / 4
            b = torch.randint(-8, 9, (Cout,), generator=g).float() / 4
        else:
            x = torch.randn(B, Cin, H, W, generator=g).half().float()
            w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)       # NOT rounded: the packers round
            b = torch.randn(Cout, generator=g) * 0.1
        _cases[key] = dict(xd=_nhwc(x).half().to(DEV), w9=pack_conv3x3(w).to(DEV), wf=pack_conv_upfold(w).to(DEV), bd=b.to(DEV), ref=_ref64(x, w, b))
    return _cases[key]


def _launch(c, wkey, B, H, W, f32view=False):
    """one launch into poisoned outputs; returns (outputs on the CPU, launches the folded form served)"""
    Cout = c["bd"].numel()
    M = 4 * B * H * W
    n0 = ops.upfold_launch_count()
    if f32view:          # fp32 rows + the fp16 copy, both as column views of wider matrices (ldc > N)
        big = torch.full((M, Cout + 64), 7.0, dtype=torch.float32, device=DEV)
        big16 = torch.full((M, Cout + 8), 7.0, dtype=torch.float16, device=DEV)
        ops.conv3x3(c["xd"], c[wkey], big[:, :Cout], B, H, W, c["bd"], upsample2x=True, out16=big16[:, :Cout])
        torch.cuda.synchronize()
        assert float((big[:, Cout:] - 7.0).abs().max()) == 0 and float((big16[:, Cout:] - 7.0).abs().max()) == 0, "wrote past the view"
        outs = (big[:, :Cout].cpu(), big16[:, :Cout].cpu())
    else:
        out = torch.full((M, Cout), 7.0, dtype=torch.float16, device=DEV)
        ops.conv3x3(c["xd"], c[wkey], out, B, H, W, c["bd"], epi=EPI_BIAS, upsample2x=True)
        torch.cuda.synchronize()
        outs = (out.cpu(),)
    return outs, ops.upfold_launch_count() - n0


def _exact(B, H, W, Cin, Cout, f32view=False):
    c = _case("exact", B, H, W, Cin, Cout)
    old, n_old = _launch(c, "w9", B, H, W, f32view)
    new, n_new = _launch(c, "wf", B, H, W, f32view)
    assert (n_old, n_new) == (0, 1), ("the folded counter must move by exactly the folded launches", n_old, n_new)
    ref = c["ref"]
    assert float(ref.abs().max()) < 60000                    # inside fp16's range: the fp16 outputs are one rounding of the exact value
    for o, n in zip(old, new):
        want = ref.float() if n.dtype == torch.float32 else ref.half()
        assert torch.equal(n, want), ("folded != fp64 reference", float((n.double() - ref).abs().max()))
        assert torch.equal(o, n), "folded != 9-tap"


#          B  H   W   Cin  Cout
SHAPES = [(2, 5, 7, 64, 64),          # tail tile (70 of 256 rows per parity), non-power-of-two map
          (3, 12, 10, 128, 192),      # several M tiles per parity (360 rows), two channel blocks, ragged N (192 of 2 x 128)
          (1, 1, 1, 64, 320),         # every window position but one masked
          (2, 4, 4, 640, 320)]        # split-K: 40 K-tiles on 8 tiles


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES[:3])
@pytest.mark.parametrize("bm128", [0, 1], ids=["bm256", "bm128"])
def test_exact_cases(B, H, W, Cin, Cout, bm128):
    ops.set_option(46, 4 if bm128 else 0)           # key 46 bit 2: half-height tiles for every conv whose 256-row grid covers at most half the chip
    ops.set_option(34, 1000)                        # no split-K
    try:
        assert _plan(B, H, W, Cin, Cout) == (128 if bm128 else 256, 1)
        _exact(B, H, W, Cin, Cout)
    finally:
        ops.set_option(46, DEFAULTS[46])
        ops.set_option(34, DEFAULTS[34])


@pytest.mark.parametrize("minkt", [10, 20])
def test_exact_split_k(minkt):
    """key 34 = the minimum K-tiles per slice: 40 K-tiles on an 8-tile grid are cut into 4 / 2 slices; the partial tiles sit in the workspace
    in OUTPUT-row order and the unchanged reduction applies bias and stores"""
    B, H, W, Cin, Cout = SHAPES[3]
    ops.set_option(34, minkt)
    try:
        assert _plan(B, H, W, Cin, Cout)[1] == 40 // minkt
        _exact(B, H, W, Cin, Cout)
        _exact(B, H, W, Cin, Cout, f32view=True)
    finally:
        ops.set_option(34, DEFAULTS[34])


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES[:3])
def test_exact_fp32_rows_with_fp16_copy_into_column_views(B, H, W, Cin, Cout):
    _exact(B, H, W, Cin, Cout, f32view=True)


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES[:2])
def test_random_values_against_fp64(B, H, W, Cin, Cout):
    c = _case("random", B, H, W, Cin, Cout)
    (old,), n_old = _launch(c, "w9", B, H, W)
    (new,), n_new = _launch(c, "wf", B, H, W)
    assert (n_old, n_new) == (0, 1)
    ref = c["ref"]
    r_new = float((new.double() - ref).norm() / ref.norm())
    r_old = float((old.double() - ref).norm() / ref.norm())
    print(f"[upfold {B}x{H}x{W} {Cin}->{Cout}] rel-L2 to the fp64 conv: folded {r_new:.3e}, 9-tap {r_old:.3e}")
    assert torch.isfinite(new).all() and r_new < 1e-3, r_new


def test_bad_arguments():
    B, H, W, Cin, Cout = 2, 5, 7, 64, 64
    c = _case("exact", B, H, W, Cin, Cout)
    out = torch.empty(4 * B * H * W, Cout, dtype=torch.float16, device=DEV)
    out32 = torch.empty(B, Cout, 2 * H, 2 * W, dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=DEV)

    def args():
        a = _lib.ConvArgs()
        a.inp = c["xd"].data_ptr()
        a.B, a.Hin, a.Win, a.Cin, a.Hout, a.Wout, a.stride, a.upsample2x = B, H, W, Cin, 2 * H, 2 * W, 1, 2
        a.g.w, a.g.bias, a.g.N, a.g.epi = c["wf"].data_ptr(), c["bd"].data_ptr(), Cout, EPI_BIAS
        a.g.out, a.g.ldc, a.g.out_mode = out.data_ptr(), Cout, OUT_F16_ROWMAJOR
        a.g.workspace, a.g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        return a

    st = torch.cuda.current_stream().cuda_stream
    call = lambda a: _lib.lib().gl_conv3x3(C.byref(a), st)
    n0 = ops.upfold_launch_count()
    assert call(args()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), c["ref"].half())
    for field, val in (("stride", 2), ("in_split", 2), ("w_split", 1), ("upsample2x", 3)):
        a = args()
        setattr(a, field, val)
        if field == "stride":
            a.Hout, a.Wout = H, W
        assert call(a) == -1, field
    a = args()
    a.g.out, a.g.ldc, a.g.out_mode, a.g.hw = out32.data_ptr(), 0, OUT_F32_NCHW, 4 * H * W
    assert call(a) == -1, "NCHW output"
    torch.cuda.synchronize()
    assert ops.upfold_launch_count() == n0 + 1


def _rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_tiny_engine_under_both_values_of_the_key():
    """the bound of tests/test_gpu_model.py::test_tiny_unet_matches_reference_golden (rel-L2 < 2.1e-3) for an engine created under key 55 = 1
    and one created under key 55 = 0, alive in one process; same launch count; the folded engine's up convs are counted"""
    from layoutllm_t2i_amd.arch import TINY, build_plan
    from layoutllm_t2i_amd.model import GroundingNetInput, UNetModel
    n_up = sum(l.kind == "up" for l in build_plan(TINY).all_layers())
    assert n_up == 3
    case = next(c for c in gc.CASES if c["name"] == "unet_tiny_cond")
    inp = {a: T(v) for a, v in gc.case_inputs(case).items()}
    ref = T(np.load(os.path.join(GOLD, "unet_tiny_cond.npz"))["out"])
    models = {}
    try:
        for key in (1, 0):
            ops.set_option(55, key)
            m = UNetModel(TINY, recipe.state_dict(TINY, 0), device=DEV, sd_first_conv=recipe.sd_first_conv(TINY, 0))
            m.grounding_tokenizer_input = GroundingNetInput()
            m.engine.use_graphs = False
            models[key] = m
    finally:
        ops.set_option(55, DEFAULTS[55])
    res = {}
    for key in (0, 1, 0, 1):                    # interleaved: each engine keeps the form it was created with
        m = models[key]
        m.fuser_scale, m.first_conv_type = case["scale"], "GLIGEN"
        g = m.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)
        d = dict(x=inp["x"].to(DEV), timesteps=torch.tensor(case["t"], dtype=torch.long), context=inp["context"], relations=inp["relations"],
                 inpainting_extra_input=None, grounding_extra_input=None, grounding_input=g)
        n0 = ops.upfold_launch_count()
        out = m(d).clone()
        torch.cuda.synchronize()
        served = ops.upfold_launch_count() - n0
        r = _rel_l2(out, ref)
        print(f"[unet_tiny_cond key55={key}] rel_l2={r:.3e} folded launches={served} launches={m.engine.num_launches()}")
        assert torch.isfinite(out).all() and r < 2.1e-3, (key, r)
        assert served == (n_up if key else 0), (key, served)
        if key in res:
            assert torch.equal(res[key][0], out)
        res[key] = (out, m.engine.num_launches())
    assert res[0][1] == res[1][1]
    print(f"[unet_tiny_cond] folded vs 9-tap rel_l2={_rel_l2(res[1][0], res[0][0]):.3e}")


def test_small_vae_decoder_under_both_values_of_the_key():
    """the bound of tests/test_gpu_vae.py::test_vae_tiny_matches_reference_golden (rel-L2 < 6e-3) under both values; engine == op-level mirror"""
    from layoutllm_t2i_amd.arch import VAE_TINY
    from layoutllm_t2i_amd.vae import VAEDecoder
    case = next(c for c in gc.CASES if c["name"] == "vae_tiny")
    z = T(gc.case_inputs(case)["z"])
    ref = T(np.load(os.path.join(GOLD, "vae_tiny.npz"))["out"])
    sd = recipe.vae_state_dict(VAE_TINY, 0)
    decs = {key: VAEDecoder(sd, VAE_TINY, DEV, fold_up=bool(key)) for key in (1, 0)}
    launches = {}
    for key in (0, 1):
        dec = decs[key]
        dec.use_graphs = False
        n0 = ops.upfold_launch_count()
        out = dec.decode(z)
        torch.cuda.synchronize()
        served = ops.upfold_launch_count() - n0
        r = _rel_l2(out, ref)
        print(f"[vae_tiny key55={key}] rel_l2={r:.3e} folded launches={served}")
        assert torch.isfinite(out).all() and r < 6e-3, (key, r)
        assert served == (1 if key else 0), (key, served)
        assert torch.equal(out, dec.decode_oplevel(z))
        launches[key] = _lib.lib().gl_vae_num_launches(dec.handle)
    assert launches[0] == launches[1]
