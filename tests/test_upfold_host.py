"""Upsample convs as four folded 2x2 convs (option key 55, weights.pack_conv_upfold), host side: the identity against the fp64 conv of the
nearest-upsampled map, the packed layout, the library's weight tables under both values of the key, and the packer's round trip."""
import dataclasses
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
from layoutllm_t2i_amd import _lib, recipe
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, UNetConfig, VAEConfig, build_plan, vae_decoder_param_shapes
from layoutllm_t2i_amd.vae import packed_shapes
from layoutllm_t2i_amd.weights import UPFOLD_TAPS, PackedWeights, pack_conv3x3, pack_conv_upfold, pack_state_dict

KEY = _lib.OPT_FOLD_UP


@pytest.fixture(autouse=True)
def _restore_key():
    old = _lib.lib().gl_get_option(KEY)
    yield
    _lib.check(_lib.lib().gl_set_option(KEY, old), "gl_set_option")


def _set(v):
    _lib.check(_lib.lib().gl_set_option(KEY, v), "gl_set_option")


def _fold64(w):
    """the four folded kernels of w [Cout, Cin, 3, 3] in fp64, straight from the definition: [2, 2, Cout, Cin, 2, 2]"""
    S = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    f = torch.zeros(2, 2, w.shape[0], w.shape[1], 2, 2, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    for ky in S[py, a]:
                        for kx in S[px, b]:
                            f[py, px, :, :, a, b] += w[:, :, ky, kx]
    return f


def _unpack(packed, cout, cin):
    """[4 Cout, 4 Cin] in the packed K order -> [2, 2, Cout, Cin, 2, 2]"""
    return packed.reshape(2, 2, cout, cin // 64, 2, 2, 64).permute(0, 1, 2, 3, 6, 4, 5).reshape(2, 2, cout, cin, 2, 2)


def test_tap_sets_are_the_issue_s():
    assert UPFOLD_TAPS == (((0,), (1, 2)), ((0, 1), (2,)))


@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
def test_identity_against_fp64_upsampled_conv(H, W):
    """parity (py, px) of conv2d(interpolate(x, 2, 'nearest'), w, padding=1) = the 2x2 conv with window origin (py - 1, px - 1) on the source
    map, out-of-map positions reading zero -- assembled parity by parity, max error below 1e-12"""
    g = torch.Generator().manual_seed(5 * H + W)
    B, Cin, Cout = 2, 3, 4
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    f = _fold64(w)
    got = torch.zeros_like(ref)
    for py in range(2):
        for px in range(2):
            # window rows y + py - 1 + a, a = 0, 1: pad one row above for py = 0, one below for py = 1 (columns likewise)
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            got[:, :, py::2, px::2] = F.conv2d(xp, f[py, px])
    err = float((got - ref).abs().max())
    assert got.shape == (B, Cout, 2 * H, 2 * W) and err < 1e-12, err


def test_pack_matches_the_fp64_fold_rounded_once():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(8, 128, 3, 3, generator=g) / 30.0
    got = _unpack(pack_conv_upfold(w).float(), 8, 128)
    f64 = _fold64(w.double())
    # sums of at most four fp32 terms, then ONE rounding to fp16: within one fp16 ulp-half of the exact sum (plus the fp32 summation error)
    assert float((got.double() - f64).abs().max()) <= float(f64.abs().max()) * (2.0 ** -11 + 2.0 ** -22)
    # folding the fp16-ROUNDED weights instead gives other bits somewhere: the pack folds from fp32
    assert not torch.equal(pack_conv_upfold(w), pack_conv_upfold(w.half().float()))


def test_layout_shape_k_order_parity_order():
    """row = parity * Cout + o with parity = py * 2 + px outermost; column = (channel block, tap a * 2 + b, channel in block).  Two arange-style
    weights whose folded values are small integers (exact in fp16): tap k weighs 2^k, so a folded value names the set of taps it summed; and the
    centre tap alone carries the index o * Cin + c, so a folded value names the (o, c) it belongs to."""
    Cout, Cin = 2, 128
    taps = torch.tensor([[2.0 ** (ky * 3 + kx) for kx in range(3)] for ky in range(3)])
    p = pack_conv_upfold(taps.expand(Cout, Cin, 3, 3).contiguous())
    assert p.shape == (4 * Cout, 4 * Cin) and p.dtype == torch.float16 and p.is_contiguous()
    idx = torch.zeros(Cout, Cin, 3, 3)
    idx[:, :, 1, 1] = torch.arange(Cout * Cin, dtype=torch.float32).reshape(Cout, Cin)
    q = pack_conv_upfold(idx)
    S = UPFOLD_TAPS
    for py in range(2):
        for px in range(2):
            for o in range(Cout):
                for c in range(Cin):
                    for a in range(2):
                        for b in range(2):
                            row = (py * 2 + px) * Cout + o
                            col = (c // 64) * 256 + (a * 2 + b) * 64 + (c % 64)
                            assert float(p[row, col]) == sum(2.0 ** (ky * 3 + kx) for ky in S[py][a] for kx in S[px][b]), (py, px, a, b)
                            centre = 1 in S[py][a] and 1 in S[px][b]
                            assert float(q[row, col]) == (o * Cin + c if centre else 0), (py, px, o, c, a, b)
    # the all-ones kernel: a window position sums 1, 2, 2 or 4 taps -- the four parities differ only in which corner holds which count
    ones = pack_conv_upfold(torch.ones(1, 64, 3, 3)).float().reshape(4, 4, 64)[:, :, 0]
    assert ones.tolist() == [[1, 2, 2, 4], [2, 1, 4, 2], [2, 4, 1, 2], [4, 2, 2, 1]]


def _up_layers(cfg):
    return [l for l in build_plan(cfg).all_layers() if l.kind == "up"]


@pytest.mark.parametrize("cfg", [UNetConfig(), TINY], ids=["full", "tiny"])
def test_unet_weight_table_follows_the_key_at_creation(cfg):
    ups = _up_layers(cfg)
    assert len(ups) == len(cfg.channel_mult) - 1
    tables = {}
    for key in (1, 0):
        _set(key)
        h = _lib.create_engine(cfg)
        _set(1 - key)                          # the key is read when the handle is created: a later change does not reach it
        tables[key] = {n: s for n, _, _, _, s in _lib.weight_table(h)[0]}
        assert _lib.lib().gl_destroy(h) == 0
        hs = _lib.create_engine(dataclasses.replace(cfg, split_weights=True), fold_up=bool(key))
        ts = {n: s for n, _, _, _, s in _lib.weight_table(hs)[0]}
        assert _lib.lib().gl_destroy(hs) == 0
        for l in ups:                          # a split_weights table never folds
            assert ts[l.prefix + ".w"] == (l.cout, 18 * l.cin)
    for l in ups:
        assert tables[1][l.prefix + ".w"] == (4 * l.cout, 4 * l.cin) and tables[1][l.prefix + ".b"] == (l.cout,)
        assert tables[0][l.prefix + ".w"] == (l.cout, 9 * l.cin)
    up_names = {l.prefix + ".w" for l in ups}
    assert {n for n in tables[1] if tables[1][n] != tables[0][n]} == up_names and list(tables[1]) == list(tables[0])
    # create_engine(fold_up=...) creates under the given value and leaves the process value alone
    _set(1)
    h = _lib.create_engine(cfg, fold_up=False)
    assert {n: s for n, _, _, _, s in _lib.weight_table(h)[0]} == tables[0] and _lib.fold_up_default() is True
    assert _lib.lib().gl_destroy(h) == 0


def test_default_of_the_key_handles_keep_their_tables_the_packers_fold_by_rule():
    """key 55 = 2, the default: gl_create / gl_vae_create give the 9-tap tables (a host that does not know the fold gets what it always got);
    the packers fold the configs whose narrowest up conv has at least 512 (UNet) / 256 (VAE decoder) channels -- the full models, not the tiny ones"""
    from layoutllm_t2i_amd.vae import _fold
    from layoutllm_t2i_amd.weights import fold_up_rule
    assert _lib.fold_up_option() == 2 and _lib.fold_up_default() is False
    for cfg in (UNetConfig(), TINY):
        h = _lib.create_engine(cfg)
        t = {n: s for n, _, _, _, s in _lib.weight_table(h)[0]}
        assert _lib.lib().gl_destroy(h) == 0
        for l in _up_layers(cfg):
            assert t[l.prefix + ".w"] == (l.cout, 9 * l.cin)
    assert fold_up_rule(UNetConfig()) is True and fold_up_rule(TINY) is False
    assert fold_up_rule(dataclasses.replace(UNetConfig(), split_weights=True)) is False
    assert _fold(None, VAEConfig()) is True and _fold(None, VAE_TINY) is False
    assert _lib.resolve_fold_up(None, True) is True and _lib.resolve_fold_up(False, True) is False and _lib.resolve_fold_up(True, False) is True
    P = pack_state_dict(recipe.state_dict(TINY, 0), TINY, "cpu", recipe.sd_first_conv(TINY, 0))
    assert P.fold_up is False
    for l in _up_layers(TINY):
        assert tuple(P.w[l.prefix + ".w"].shape) == (l.cout, 9 * l.cin)
    _set(1)
    assert _lib.resolve_fold_up(None, False) is True
    _set(0)
    assert _lib.resolve_fold_up(None, True) is False


@pytest.mark.parametrize("cfg", [VAEConfig(), VAE_TINY], ids=["full", "tiny"])
def test_vae_weight_table_follows_the_key_at_creation(cfg):
    shapes = vae_decoder_param_shapes(cfg)
    ups = [n[:-7] for n in shapes if n.endswith(".upsample.conv.weight")]
    assert len(ups) == len(cfg.ch_mult) - 1
    for key in (1, 0):
        _set(key)
        h = _lib.create_vae(cfg)
        _set(1 - key)
        table = {n: s for n, _, _, _, s in _lib.vae_weight_table(h)[0]}
        _lib.lib().gl_vae_destroy(h)
        want = packed_shapes(shapes, fold_up=bool(key))
        assert {n: s for n, (s, _) in want.items()} == table
        for p in ups:
            c = shapes[p + ".weight"][0]
            assert table[p + ".w"] == ((4 * c, 4 * c) if key else (c, 9 * c))


@pytest.mark.parametrize("key", [1, 0])
def test_pack_state_dict_round_trips_under_both_values(key):
    _set(key)
    sd = recipe.state_dict(TINY, 0)
    P = pack_state_dict(sd, TINY, "cpu", recipe.sd_first_conv(TINY, 0))             # fold_up = None: the current value of the key
    assert P.fold_up is bool(key)
    _set(1 - key)                                                                  # the pack remembers what it was laid out by
    Q = PackedWeights.from_flat(P.flat.clone(), TINY, "cpu", P.has_sd_conv, fold_up=P.fold_up)
    assert set(Q.w) == set(P.w) and all(torch.equal(Q.w[n], P.w[n]) for n in P.w)
    X = pack_state_dict(sd, TINY, "cpu", recipe.sd_first_conv(TINY, 0), fold_up=bool(key))
    assert torch.equal(X.flat, P.flat)
    for l in _up_layers(TINY):
        w32 = torch.from_numpy(sd[l.prefix + ".weight"]).float() if not torch.is_tensor(sd[l.prefix + ".weight"]) else sd[l.prefix + ".weight"].float()
        want = pack_conv_upfold(w32) if key else pack_conv3x3(w32)
        assert torch.equal(P.w[l.prefix + ".w"], want), l.prefix
    # a split_weights pack keeps [Whi | Wlo] 3x3 rows whatever the key says
    S = pack_state_dict(sd, dataclasses.replace(TINY, split_weights=True), "cpu", recipe.sd_first_conv(TINY, 0), fold_up=True)
    for l in _up_layers(TINY):
        assert tuple(S.w[l.prefix + ".w"].shape) == (l.cout, 18 * l.cin)
