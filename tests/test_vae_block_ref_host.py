"""tests/vae_block_ref.py checked on the CPU, before tests/test_gpu_vae_kernels.py relies on it: the helper against the pinned oracle, the
GroupNorm cases against the chunk regimes they claim (from ops.gn_nchunk alone), and "reference alone" for every toleranced comparison of
the GPU file -- what CPU fp32 arithmetic by itself does to that comparison, which bounds what a correct fp32-accumulating kernel may do."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import vae_block_ref as R
from layoutllm_t2i_amd import ops, vae
from layoutllm_t2i_amd.weights import pack_conv3x3
from oracle import vae_ref

F32, F64 = torch.float32, torch.float64
SH, SW = R.MAP


def _packed(cfgname, prefix, encoder):
    sd, need = R.block_state(cfgname, prefix, encoder)
    return sd, need, vae._pack(sd, need, "cpu")


# ------------------------------------------------------------------------------------------------------------------ helper == oracle
@pytest.mark.parametrize("stage,cfgname,p,cin,cout", [R.RESNET_CASES[1], R.RESNET_CASES[4], R.RESNET_CASES[5], ("dec", "tiny", "decoder.mid.block_1", 128, 128)])
def test_plain_resnet_block_equals_oracle_fp64(stage, cfgname, p, cin, cout):
    sd, need = R.block_state(cfgname, p, stage == "enc")
    x = R.rnd(f"ho.{p}", (R.B * SH * SW, cin)) * 1.2 + 0.2
    out = R.resnet_block(R.pack_exact(sd, need), p, x, R.B, SH, SW, False)
    osd = {k: torch.as_tensor(v).double() for k, v in sd.items()}
    ref = R.nhwc_rows(vae_ref.resnet_block(osd, p, R.nchw(x.double(), R.B, SH, SW)))
    assert out.dtype == F64 and out.shape == (R.B * SH * SW, cout)
    assert float((out - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("stage,cfgname,p,C", R.ATTN_BLOCK_CASES)
def test_plain_attn_block_equals_oracle_fp64(stage, cfgname, p, C):
    """also the q fold: the oracle scales the logits by C^-0.5, the helper gets q weights and bias that carry it"""
    sd, need = R.block_state(cfgname, p, False)
    N = SH * SW
    x = R.rnd(f"ho.{p}.{C}", (R.B * N, C)) * 1.2 + 0.2
    out = R.attn_block(R.pack_exact(sd, need), p, x, R.B, N, False)
    osd = {k: torch.as_tensor(v).double() for k, v in sd.items()}
    ref = R.nhwc_rows(vae_ref.attn_block(osd, p, R.nchw(x.double(), R.B, SH, SW)))
    assert float((out - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("cfgname,p,encoder", [("full", "decoder.up.0.block.0", False), ("tiny", "decoder.mid.attn_1", False),
                                               ("full", "encoder.down.1.block.0", True)])
def test_pack_exact_has_the_packers_layout(cfgname, p, encoder):
    """pack_exact is vae._pack without the fp16 rounding: rounded, it IS the packer's output (q: to one fp16 ulp, subnormals included: the packer folds in fp32)"""
    sd, need, W = _packed(cfgname, p, encoder)
    E = R.pack_exact(sd, need)
    assert set(E) == set(W)
    for k, w in W.items():
        if k.endswith("attn_1.q.w") or k.endswith("attn_1.q.b"):
            assert torch.allclose(w.double(), E[k], rtol=2.0 ** -9, atol=2.0 ** -24), k
        else:
            assert torch.equal(w, E[k].to(w.dtype)), k


def test_unpack_conv3x3_inverts_the_packer():
    w = R.rnd("unp", (96, 192, 3, 3))
    assert torch.equal(R.unpack_conv3x3(pack_conv3x3(w), F32), w.half().float())
    w3 = R.rnd("unp3", (32, 3, 3, 3))
    u = R.unpack_conv3x3(pack_conv3x3(w3, 64), F32)
    assert torch.equal(u[:, :3], w3.half().float()) and float(u[:, 3:].abs().max()) == 0.0


def test_round_points_are_the_engines():
    """round_points=True differs from the plain block by fp16 roundings only (a few 1e-4 relative), and its output is fp16-representable"""
    sd, need, W = _packed("full", "decoder.up.0.block.0", False)
    x = R.block_input("rp", R.B * SH * SW, 256)
    a, b = R.resnet_block(W, "decoder.up.0.block.0", x, R.B, SH, SW, True), R.resnet_block(W, "decoder.up.0.block.0", x, R.B, SH, SW, False)
    assert torch.equal(a, a.half().double()) and not torch.equal(b, b.half().double())
    assert 5e-5 < float((a - b).norm() / b.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------------------------ GroupNorm regimes
def test_groupnorm_cases_reach_the_chunk_regimes():
    n = {hw: ops.gn_nchunk(hw) for _, hw in R.GN_CASES}
    assert n[4096] == 64                                                         # the UNet's regime, kept as the control
    assert (n[4100],) + R.gn_chunks(4100, n[4100]) == (8, 513, 509, 0)           # HW > 4096: short last chunk
    assert (n[33856],) + R.gn_chunks(33856, n[33856]) == (66, 513, 511, 0)       # more than 64 chunks, short last chunk
    assert (n[130],) + R.gn_chunks(130, n[130]) == (32, 5, 5, 6)                 # trailing EMPTY chunks
    assert max(n.values()) > 64 and any(R.gn_chunks(hw, c)[2] > 0 for hw, c in n.items())
    assert any(R.gn_chunks(hw, c)[1] < R.gn_chunks(hw, c)[0] for hw, c in n.items())
    for C, hw in R.GN_SHARP_CASES:
        assert (C, hw) in R.GN_CASES and not R.gn_single_launch(C, hw)           # the sharp cases all take statistics + apply
    assert {(C, hw) for C, hw in R.GN_CASES if R.gn_single_launch(C, hw)} == {(256, 768), (256, 769), (256, 1280), (256, 1281), (256, 2560),
                                                                                 (512, 384), (512, 385), (512, 1280)}
    assert {C // 32 for C, _ in R.GN_CASES} == {2, 4, 8, 16}


# ------------------------------------------------------------------------------------------------------------------ reference alone
def _ratio(out, ref, tol):
    r = R.worst_ratio(out, ref, *tol)
    print(f"CPU fp32 against fp64: {r:.3f} of rtol {tol[0]:g} / atol {tol[1]:g}")
    return r


@pytest.mark.parametrize("C,HW", R.GN_CASES)
def test_reference_alone_groupnorm(C, HW):
    """test_groupnorm_vae_widths (1e-3 / 1e-4, fp16 output against the unrounded fp64 op) and, for the sharp cases, the 2e-5 / 2e-6
    comparison of hi + lo with both input kinds: the op in CPU fp32 passes with the 4x margin"""
    g, b = R.gn_affine(C)
    kinds = [(False, True, R.KERNEL_TOL)]
    if (C, HW) in R.GN_SHARP_CASES:
        kinds += [(False, True, R.GN_SHARP_TOL), (True, False, R.GN_SHARP_TOL)]
    for large_mean, silu, tol in kinds:
        x = R.gn_input(C, HW, large_mean)
        x = R.r16(x) if tol is R.KERNEL_TOL else x
        assert _ratio(R.group_norm(x, g, b, R.B, HW, silu), R.group_norm(x.double(), g, b, R.B, HW, silu), tol) <= 0.25


def test_reference_alone_gemm_and_conv():
    """test_vae_gemm_and_conv_shapes: the longest sums of the file (K = 512 GEMM, K = 4608 conv) at 1e-3 / 1e-4, and both out convs at the
    fp32-output tolerance 1e-4 / 1e-5"""
    M = R.B * SH * SW
    a, w, b = R.gemm_operands(512, 512, M)
    assert _ratio(F.linear(a, w, b), F.linear(a.double(), w.double(), b.double()), R.KERNEL_TOL) <= 0.25
    for (cin, cout), tol in [((512, 512), R.KERNEL_TOL)] + [(c, R.CONV_OUT_TOL) for c in R.CONV_OUT_CASES]:
        x, w4, b = R.conv_operands(cin, cout, R.B, SH, SW)
        assert _ratio(R.conv3x3(x, w4, b, R.B, SH, SW), R.conv3x3(x.double(), w4.double(), b.double(), R.B, SH, SW), tol) <= 0.25


@pytest.mark.parametrize("C,N", R.ATTN_CASES)
def test_reference_alone_attention_steps_and_chain(C, N):
    """test_vae_attention_chain_per_kernel.  Per step (each judged on that step's own inputs, unrounded output): logits and P.V at 1e-3 / 1e-4,
    softmax at rtol 2e-3 / atol 1e-6 -- CPU fp32 passes with the 4x margin.  Whole chain against exact fp64 attention: the rounded model in
    CPU fp32 stays under ATTN_CHAIN_CPU_FIGURE of 2e-3 / 2e-4 at ATTN_CHAIN_LOGIT_STD, and does not reach the 4x margin at a quarter of
    that scale either, which is why that comparison's tolerance is widened (vae_block_ref.attn_chain_tol)."""
    q, k, v = R.attn_inputs(C, N, R.ATTN_CHAIN_LOGIT_STD)
    s = slice(0, N)
    l32, l64 = q[s] @ k[s].T, q[s].double() @ k[s].double().T
    assert _ratio(l32, l64, R.KERNEL_TOL) <= 0.25
    lh = R.r16(l32)
    p32, p64 = torch.softmax(lh, -1), torch.softmax(lh.double(), -1)
    assert float(((p32.double() - p64).abs() / (1e-6 + 2e-3 * p64)).max()) <= 0.25
    ph = R.r16(p32)
    assert _ratio(ph @ v[s], ph.double() @ v[s].double(), R.KERNEL_TOL) <= 0.25
    exact = R.attention(q.double(), k.double(), v.double(), R.ATTN_B, N, False)
    fig = _ratio(R.attention(q, k, v, R.ATTN_B, N, True), exact, R.ATTN_TOL)
    assert fig <= R.ATTN_CHAIN_CPU_FIGURE
    if (C, N) == (512, 64):          # the case that sets the figure: no smaller scale gives the margin
        for std in (R.ATTN_CHAIN_LOGIT_STD, R.ATTN_CHAIN_LOGIT_STD / 2, R.ATTN_CHAIN_LOGIT_STD / 4):
            q2, k2, v2 = R.attn_inputs(C, N, std)
            e2 = R.attention(q2.double(), k2.double(), v2.double(), R.ATTN_B, N, False)
            assert _ratio(R.attention(q2, k2, v2, R.ATTN_B, N, True), e2, R.ATTN_TOL) > 0.25
    assert R.attn_chain_tol() == (2e-3 * 4 * R.ATTN_CHAIN_CPU_FIGURE, 2e-4 * 4 * R.ATTN_CHAIN_CPU_FIGURE)


def test_hard_logits_inputs():
    """the hard-logits case really has row maxima near ATTN_HARD_ROWMAX, inside fp16's range with room to spare"""
    C, N = R.ATTN_HARD_CASE
    q, k, v = R.attn_hard_inputs(C, N)
    mx = torch.stack([(q[b * N:(b + 1) * N].double() @ k[b * N:(b + 1) * N].double().T).max(1).values for b in range(R.ATTN_B)])
    assert abs(float(mx.median()) - R.ATTN_HARD_ROWMAX) < 0.5 and 25 < float(mx.min()) and float(mx.max()) < 80


@pytest.mark.parametrize("stage,cfgname,p,cin,cout", R.RESNET_CASES)
def test_reference_alone_resnet_blocks(stage, cfgname, p, cin, cout):
    """test_vae_blocks_vs_rounded_fp64_model: the rounded model in CPU fp32 against the rounded model in fp64 stays under its kind's
    BLOCK_CPU_FIGURE; the figure is above 0.25 (no 4x margin, at this input scale or a quarter of it), so block_tol() widens"""
    _, _, W = _packed(cfgname, p, stage == "enc")
    kind = R.block_kind(cin, cout)
    figs = []
    for scale in (1.0, 0.25):
        x = R.r16(R.block_input(p, R.B * SH * SW, cin) * scale)
        figs.append(_ratio(R.resnet_block(W, p, x, R.B, SH, SW, True, F32), R.resnet_block(W, p, x, R.B, SH, SW, True), R.BLOCK_TOL))
    assert figs[0] <= R.BLOCK_CPU_FIGURE[kind]
    assert min(figs) > 0.25 and R.block_tol(kind)[0] == 1e-3 * 4 * R.BLOCK_CPU_FIGURE[kind]


@pytest.mark.parametrize("stage,cfgname,p,C", R.ATTN_BLOCK_CASES)
def test_reference_alone_attn_blocks(stage, cfgname, p, C):
    _, _, W = _packed(cfgname, p, False)
    N = SH * SW
    figs = []
    for scale in (1.0, 0.25):
        x = R.r16(R.block_input(p + cfgname, R.B * N, C) * scale)
        figs.append(_ratio(R.attn_block(W, p, x, R.B, N, True, F32), R.attn_block(W, p, x, R.B, N, True), R.BLOCK_TOL))
    assert figs[0] <= R.BLOCK_CPU_FIGURE["attn"]
    assert min(figs) > 0.25 and R.block_tol("attn")[0] == 1e-3 * 4 * R.BLOCK_CPU_FIGURE["attn"]
