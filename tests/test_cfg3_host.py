"""Separate text and layout guidance scales (three-branch CFG), everything that needs no GPU: the float64 restatement (tests/cfg3_ref.py),
``interface.check_layout_guidance``, the argument checks of ``gl_cfg3_combine`` and the struct of ``gl_cfg3_eval``, and the three samplers on
a recording engine -- which engine entries a run issues, with which arguments, how often the conditioning is set and in which form, and
that the torch RNG stream does not notice the key."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import cfg3_ref as c3
import norel_cases as nc
import sem_cases as semc
import sp_cases as sc
import stubs
from layoutllm_t2i_amd import _lib, host, recipe, txt2img
from layoutllm_t2i_amd import gligen_inference as gi
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import sampler as sampler_mod
from layoutllm_t2i_amd import train_rl
from layoutllm_t2i_amd.arch import TINY
from layoutllm_t2i_amd.family import family_of
from layoutllm_t2i_amd.model import GroundingNetInput, LatentDiffusion, UNetModel
from layoutllm_t2i_amd.sampler import SAMPLER_KEYS, DDIMSampler, DPMSolverSampler, PLMSSampler, resolve_sampler

KEY = "layout_guidance_scale"


# ------------------------------------------------------------------------------------------- the formula
def test_fp64_combine_reduces_to_the_two_branch_forms():
    rng = np.random.default_rng(0)
    e_c, e_t, e_u = (rng.standard_normal((2, 4, 8, 8)) for _ in range(3))
    for s in (7.5, 1.0, 12.0):
        assert np.abs(c3.combine3(e_c, e_t, e_u, s, s) - c3.combine2(e_c, e_u, s)).max() < 1e-12
        # s_l = 0: the layout is ignored, the guidance of the text-only branch remains
        assert np.array_equal(c3.combine3(e_c, e_t, e_u, s, 0.0), c3.combine2(e_t, e_u, s))
    assert np.abs(c3.combine3(e_c, e_t, e_u, 7.5, 12.0) - c3.combine2(e_c, e_u, 7.5)).max() > 1.0, "another scale is another result"
    # the rule of the steps
    assert c3.needs_text_branch(True, 0.0) and c3.needs_text_branch(False, 0.3) and not c3.needs_text_branch(False, 0.0)
    # ... which is the sampler's
    for cfg in (TINY, nc.NR_TINY):
        s = PLMSSampler(LatentDiffusion(), UNetModel.from_packed(None, cfg, "cpu"))
        for scale in (0, 0.0, 0.3, 1.0):
            assert s._needs_text_branch(scale) == c3.needs_text_branch(cfg.relation, scale)


# ------------------------------------------------------------------------------------------- validation
def test_check_layout_guidance_values():
    assert itf.check_layout_guidance(None) is None
    for v, want in ((0, 0.0), (7.5, 7.5), (3, 3.0), (np.float32(2.5), 2.5), (np.int64(4), 4.0)):
        got = itf.check_layout_guidance(v, family_of(TINY))
        assert got == want and type(got) is float
    for bad in (True, False, float("nan"), float("inf"), -float("inf"), -1, -0.5, "7.5", [7.5], np.bool_(True)):
        with pytest.raises(ValueError, match=KEY):
            itf.check_layout_guidance(bad)
    for cfg in (TINY, nc.NR_TINY, nc.NR_TI_TINY, nc.NR_IP_TINY):
        assert itf.check_layout_guidance(2.0, family_of(cfg)) == 2.0
    for cfg in (sc.CANNY_TINY, sc.HED_TINY, semc.SEM_TINY):
        assert itf.check_layout_guidance(None, family_of(cfg)) is None
        with pytest.raises(ValueError, match=KEY):
            itf.check_layout_guidance(2.0, family_of(cfg))
    # the key is no part of the sampler switch
    assert KEY not in SAMPLER_KEYS and KEY not in resolve_sampler({KEY: 3.0})[1]


class _Untouchable:
    """a model whose every attribute but ``cfg`` is an error"""
    def __init__(self, cfg):
        object.__setattr__(self, "cfg", cfg)

    def __getattr__(self, name):
        raise AssertionError(f"model.{name} read before the key was refused")


@pytest.mark.parametrize("cfg", [sc.CANNY_TINY, semc.SEM_TINY], ids=["spatial", "sem"])
def test_map_families_refuse_the_key_before_the_model_is_touched(cfg):
    am = (_Untouchable(cfg), None, None, None, {})
    noise = torch.zeros(1, 4, 16, 16)
    for entry, meta in ((itf.run_one_image, dict(prompt="a house")), (itf.run_batch_images, dict(prompts=["a house"]))):
        with pytest.raises(ValueError, match=KEY):
            entry(am, {"batch_size": 1, "guidance_scale": 7.5, KEY: 3.0}, meta, noise)
    assert am[4] == {}, "refused before the cached config was touched"
    with pytest.raises(ValueError, match=KEY):
        itf.denoise(am, None, None, None, None, noise, layout_guidance_scale=3.0)


def test_bad_values_are_refused_at_every_public_entry():
    am = (_Untouchable(TINY), None, None, None, {})
    noise = torch.zeros(1, 4, 16, 16)
    for bad in (True, -1.0, float("nan"), "3"):
        with pytest.raises(ValueError, match=KEY):
            itf.run_one_image(am, {"batch_size": 1, "guidance_scale": 7.5, KEY: bad}, dict(prompt="p", phrases=[], locations=[]), noise)
        with pytest.raises(ValueError, match=KEY):
            itf.denoise(am, None, None, None, None, noise, layout_guidance_scale=bad)
        with pytest.raises(ValueError, match=KEY):
            txt2img.generate(am, None, None, "p", None, None, layout_guidance_scale=bad)
        with pytest.raises(ValueError, match=KEY):
            train_rl.generate_with(am, layout_guidance_scale=bad)
    assert am[4] == {}


def test_public_entries_hand_the_key_on_per_call(monkeypatch):
    seen = []

    def fake_denoise(all_models, context, uc, relations, batch, noise, *a, **k):
        seen.append(dict(k))
        return noise
    grounding = lambda meta, clip, proc, bs, device=None: dict(boxes=torch.zeros(bs, 30, 4), masks=torch.zeros(bs, 30),
                                                               text_embeddings=torch.zeros(bs, 30, 768))
    monkeypatch.setattr(itf, "denoise", fake_denoise)
    monkeypatch.setattr(itf, "prepare_batch", grounding)
    monkeypatch.setattr(itf, "prepare_batch_multiple", grounding)
    stubs.install_fake_sng_parser()

    class _Decoder:
        def decode(self, z):
            return torch.zeros(z.shape[0], 3, 4, 4)
    m = type("M", (), {})()
    m.cfg = nc.NR_TINY
    am = (m, _Decoder(), stubs.StubTextEncoder(), None, {})
    noise = torch.zeros(2, 4, 16, 16)
    base = dict(batch_size=2, guidance_scale=7.5, no_plms=False)
    meta = dict(prompt="cat sitting on mat", phrases=["cat"], locations=[[0, 0, 1, 1]])
    itf.run_one_image(am, dict(base, **{KEY: 12}), dict(meta), noise)
    itf.run_one_image(am, dict(base), dict(meta), noise)                      # the cached config still holds the key: the call decides
    itf.run_one_image(am, dict(base, **{KEY: None}), dict(meta), noise)
    bmeta = dict(prompts=[meta["prompt"]] * 2, phrases=[["cat"]] * 2, locations=[[[0, 0, 1, 1]]] * 2)
    itf.run_batch_images(am, dict(base, sampler="ddim", **{KEY: 0}), bmeta, noise)
    assert seen[0][KEY] == 12.0 and type(seen[0][KEY]) is float
    assert KEY not in seen[1] and KEY not in seen[2], "absent or None: denoise is called as it always was"
    assert seen[3][KEY] == 0.0 and seen[3]["sampler"] == "ddim"
    # train_rl's adaptor routes through run_batch_images, as for sampler=
    calls = []
    monkeypatch.setattr(itf, "run_batch_images", lambda am_, args, meta_, noise_, *a, **k: calls.append(dict(args)) or [])
    monkeypatch.setattr(itf, "latent_hw", lambda *a: (16, 16))
    train_rl.generate_with(am, device="cpu", layout_guidance_scale=9)(["a cat"], [["cat"]], [[[0, 0, 1, 1]]])
    assert calls[0][KEY] == 9.0 and "sampler" not in calls[0]
    # gligen_inference.run forwards the config key when present, and only then
    got = []
    monkeypatch.setattr(itf, "run_one_image", lambda am_, args, m_, noise_, clip, proc, device=None: got.append(dict(args)) or [])
    monkeypatch.setitem(gi._MODELS, "ck", (type("M", (), {"first_conv_type": "SD"})(), None, None, None, {}))
    gmeta = dict(ckpt="ck", prompt="p", phrases=["a"], locations=[[0, 0, 1, 1]])
    gi.run(gmeta, {"batch_size": 1, "device": "cpu", KEY: 4.0}, noise[:1], clip_model=object(), clip_processor=object())
    gi.run(gmeta, dict(batch_size=1, device="cpu"), noise[:1], clip_model=object(), clip_processor=object())
    assert got[0][KEY] == 4.0 and KEY not in got[1]


# ------------------------------------------------------------------------------------------- the C entries, without a GPU
def test_cfg3_combine_refuses_bad_arguments_without_a_device():
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float))
    assert lib.gl_cfg3_combine(p, 7.5, 12.0, 0, p, None) == -1
    assert lib.gl_cfg3_combine(p, 7.5, 12.0, -4, p, None) == -1
    assert lib.gl_cfg3_combine(None, 7.5, 12.0, 4, p, None) == -1
    assert lib.gl_cfg3_combine(p, 7.5, 12.0, 4, None, None) == -1


def test_cfg3_eval_struct_and_abi():
    lib = _lib.lib()
    assert lib.gl_sizeof_cfg3_eval_args() == ctypes.sizeof(_lib.Cfg3EvalArgs)
    assert lib.gl_abi_version() == 15 == _lib.ABI_VERSION
    names = [f[0] for f in _lib.Cfg3EvalArgs._fields_]
    step = [f[0] for f in _lib._STEP_EVAL]
    assert names == ["x", "e_out", *step, "s_text", "s_layout", "use_graph"], "the evaluation's fields are the step structs'"
    a = _lib.Cfg3EvalArgs()
    assert lib.gl_cfg3_eval(None, ctypes.byref(a), None) == -1 and lib.gl_cfg3_eval(None, None, None) == -1


# ------------------------------------------------------------------------------------------- the samplers on a recording engine
class _Engine:
    """records every entry the sampler issues; evaluates nothing"""

    def __init__(self, log):
        self.log = log

    def buf(self, tag, shape, dtype=torch.float32, zero=False):
        return torch.zeros(tuple(shape), dtype=dtype)

    def set_conditioning(self, context, relations, boxes, masks, positive_embeddings, hw, **kw):
        self.log.append(("condition", dict(context=context.clone(), relations=None if relations is None else relations.clone(), boxes=boxes.clone(),
                                           masks=masks.clone(), positive_embeddings=positive_embeddings.clone(), hw=hw)))

    def plms_step(self, x_eval, x_base, x_out, e_out, e_terms, coefs, div, t, reps, guidance, fuser_scale, sd_conv, *sched):
        self.log.append(("plms_step", dict(t=t, reps=reps, guidance=guidance, fuser_scale=fuser_scale, sd_conv=sd_conv, coefs=tuple(coefs), div=div,
                                           n_terms=len(e_terms), sched=sched)))
        return x_out

    def ddim_step(self, x, x_out, **kw):
        self.log.append(("ddim_step", {k: v for k, v in kw.items() if k != "noise"}))
        return x_out

    def dpmpp_step(self, x, x_out, x0_out, **kw):
        self.log.append(("dpmpp_step", {k: v for k, v in kw.items() if k != "x0_old"}))
        return x_out

    def cfg3_eval(self, x, e_out, **kw):
        self.log.append(("cfg3_eval", dict(kw)))
        return e_out


def _model(cfg, log):
    """the real UNetModel (its ``condition``, its first-conv switch) around the recording engine, on the CPU"""
    m = UNetModel.from_packed(None, cfg, "cpu", allow_missing_sd_conv=True)
    m.engine = _Engine(log)
    m.grounding_tokenizer_input = GroundingNetInput()
    return m


def _ops_spy(monkeypatch, log):
    """the op-level updates the three-branch steps use, and the masked blend: recorded, not run (they need a GPU)"""
    def spy(name):
        def f(*a, **kw):
            log.append((name, {k: v for k, v in kw.items() if not torch.is_tensor(v)}))
        return f
    for name in ("plms_update", "ddim_update", "dpmpp_update", "latent_blend"):
        monkeypatch.setattr(sampler_mod.ops, name, spy(name))


SAMPLERS = {"plms": (PLMSSampler, {}, "plms_step", "plms_update"), "ddim": (DDIMSampler, dict(eta=0.5), "ddim_step", "ddim_update"),
            "dpmpp_2m": (DPMSolverSampler, {}, "dpmpp_step", "dpmpp_update")}
S, G, SL, B = 6, 7.5, 12.0, 2
ALPHA = [0.5, 0.0, 0.5]


def _inputs(cfg):
    return {k: torch.from_numpy(v) for k, v in recipe.synth_inputs(cfg, B, 8, n_boxes=3, n_rel=2, seed=5).items()}


def _run(monkeypatch, name, cfg, layout="absent", mask=False, explicit_none=False):
    log = []
    _ops_spy(monkeypatch, log)
    cls, kw, _, _ = SAMPLERS[name]
    model = _model(cfg, log)
    inp = _inputs(cfg)
    s = cls(LatentDiffusion(), model, alpha_generator_func=lambda n: host.alpha_generator(n, ALPHA), set_alpha_scale=itf.set_alpha_scale, **kw)
    g = model.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)
    input = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], relations=inp["relations"], grounding_input=g)
    more = dict(mask=torch.ones(1, 1, 8, 8), x0=torch.zeros(1, 4, 8, 8)) if mask else {}
    torch.manual_seed(11)
    if layout == "absent":
        s.sample(S=S, shape=tuple(inp["x"].shape), input=input, uc=inp["uc"], guidance_scale=G, **more)
    else:
        s.sample_layout(S=S, shape=tuple(inp["x"].shape), input=input, uc=inp["uc"], guidance_scale=G, layout_guidance_scale=layout, **more)
    return log, torch.get_rng_state(), inp, s


def _steps(log):
    return [e for e in log if e[0] not in ("condition", "latent_blend")]


def _evals(name, s):
    """(t, fuser scale) of every UNet evaluation of a run, in order: PLMS evaluates step 0 twice, the second time at the next timestep"""
    ts = [float(t) for t in np.flip(s.ddim_timesteps)]
    alphas = host.alpha_generator(len(ts), ALPHA)
    ev = list(zip(ts, alphas))
    if name == "plms":
        ev.insert(1, (ts[1], alphas[0]))
    return ev


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_key_absent_is_todays_call_sequence(monkeypatch, name):
    step = SAMPLERS[name][2]
    log, _, inp, s = _run(monkeypatch, name, nc.NR_TINY)
    log_none, _, _, _ = _run(monkeypatch, name, nc.NR_TINY, layout=None)          # None through the new entry: the same calls
    ev = _evals(name, s)
    assert len(ev) >= S and any(a == 0 for _, a in ev) and any(a != 0 for _, a in ev)
    for lg in (log, log_none):
        conds = [e[1] for e in lg if e[0] == "condition"]
        assert len(conds) == 1 and conds[0]["context"].shape[0] == 2 * B, "condition once, with the 2B batch"
        st = _steps(lg)
        assert [e[0] for e in st] == [step] * len(ev), "no cfg3_eval, no op-level update: the fused step alone"
        assert [(e[1]["t"], e[1]["fuser_scale"]) for e in st] == ev
        assert all(e[1]["reps"] == 2 and e[1]["guidance"] == G for e in st)
        seen_zero = False
        for e in st:                                   # the SD conv would be switched in for good at the first scale-0 step (not restorable here)
            seen_zero = seen_zero or e[1]["fuser_scale"] == 0
            assert e[1]["sd_conv"] is False
    assert [(e[0], {k: v for k, v in e[1].items() if k != "sched"}) for e in _steps(log)] == \
           [(e[0], {k: v for k, v in e[1].items() if k != "sched"}) for e in _steps(log_none)]


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_key_set_without_relations_switches_the_conditioning_once(monkeypatch, name):
    _, _, step, update = SAMPLERS[name]
    log, _, inp, s = _run(monkeypatch, name, nc.NR_TINY, layout=SL)
    ev = _evals(name, s)
    n_on = sum(1 for _, a in ev if a != 0)
    assert 0 < n_on < len(ev)
    # the order of everything: condition(3B), the fuser-on steps as cfg3_eval + update, condition(2B), the fuser-off steps as the fused step
    names = [e[0] for e in log if e[0] != "latent_blend"]
    assert names == ["condition"] + ["cfg3_eval", update] * n_on + ["condition"] + [step] * (len(ev) - n_on)
    conds = [e[1] for e in log if e[0] == "condition"]
    assert [c["context"].shape[0] for c in conds] == [3 * B, 2 * B]
    st = _steps(log)
    evals = [e for e in st if e[0] in ("cfg3_eval", step)]
    assert [(e[1]["t"], e[1]["fuser_scale"]) for e in evals] == ev
    for e in evals:
        if e[0] == "cfg3_eval":
            assert e[1]["s_text"] == G and e[1]["s_layout"] == SL and e[1]["fuser_scale"] != 0 and set(e[1]) == {"t", "fuser_scale", "sd_conv", "s_text", "s_layout"}
        else:
            assert e[1]["reps"] == 2 and e[1]["guidance"] == G and e[1]["fuser_scale"] == 0
    # [cond ; text-only ; uncond]: the middle third has the conditional context and the unconditional third's (null) grounding
    c3b, c2b = conds
    ctx, uc = inp["context"].float(), inp["uc"].float()
    assert torch.equal(c3b["context"], torch.cat([ctx, ctx, uc], 0)) and torch.equal(c2b["context"], torch.cat([ctx, uc], 0))
    for k, real in (("boxes", inp["boxes"]), ("masks", inp["masks"]), ("positive_embeddings", inp["positive_embeddings"])):
        z = torch.zeros_like(real.float())
        assert real.abs().sum() > 0
        assert torch.equal(c3b[k], torch.cat([real.float(), z, z], 0)), k
        assert torch.equal(c2b[k], torch.cat([real.float(), z], 0)), k
    assert c3b["relations"] is None


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_key_set_with_relations_runs_three_branches_on_every_step(monkeypatch, name):
    _, _, step, update = SAMPLERS[name]
    log, _, inp, s = _run(monkeypatch, name, TINY, layout=SL)
    ev = _evals(name, s)
    names = [e[0] for e in log]
    assert names == ["condition"] + ["cfg3_eval", update] * len(ev)
    cond = log[0][1]
    rel = inp["relations"].float()
    assert cond["context"].shape[0] == 3 * B and torch.equal(cond["relations"], torch.cat([rel, rel, rel], 0)), "every third reads the same relations"
    assert [(e[1]["t"], e[1]["fuser_scale"]) for e in log if e[0] == "cfg3_eval"] == ev
    # guidance_scale == 1 still runs three branches; without uc there is nothing to run them on
    model = _model(TINY, [])
    smp = SAMPLERS[name][0](LatentDiffusion(), model, **SAMPLERS[name][1])
    with pytest.raises(ValueError, match="uc"):
        smp.sample_layout(S=S, shape=(B, 4, 8, 8), input=dict(x=torch.zeros(B, 4, 8, 8)), uc=None, guidance_scale=1, layout_guidance_scale=SL)
    assert model.engine.log == []


@pytest.mark.parametrize("mask", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_rng_stream_does_not_notice_the_key(monkeypatch, name, mask):
    for cfg in (nc.NR_TINY, TINY):
        _, absent, _, _ = _run(monkeypatch, name, cfg, mask=mask)
        log, keyed, _, _ = _run(monkeypatch, name, cfg, layout=SL, mask=mask)
        assert any(e[0] == "cfg3_eval" for e in log)
        assert torch.equal(absent, keyed), "the same draws in the same order, whatever the key"
    torch.manual_seed(11)
    if name != "dpmpp_2m" or mask:
        assert not torch.equal(torch.get_rng_state(), keyed), "(the run does draw)"


def test_three_branch_updates_take_the_two_branch_coefficients(monkeypatch):
    """the scalars the op-level update gets on a three-branch step are those the fused step gets on the same step of a two-branch run"""
    for name, (_, _, step, update) in SAMPLERS.items():
        plain, _, _, _ = _run(monkeypatch, name, TINY)
        keyed, _, _, _ = _run(monkeypatch, name, TINY, layout=SL)
        a = [e[1] for e in plain if e[0] == step]
        b = [e[1] for e in keyed if e[0] == update]
        assert len(a) == len(b) > 0
        if name == "plms":
            continue                                                    # plms_update takes its scalars by position (checked on the GPU, bitwise)
        for p, k in zip(a, b):
            scalars = [key for key in k if key not in ("guidance", "noise", "x0_old", "pred_x0")]
            assert len(scalars) >= 4
            for key in scalars:
                assert p[key] == k[key], (name, key)
