"""Image-to-image (SDEdit: sampling from a noised input image, ``strength``), everything that needs no GPU: ``host.check_strength`` and
``host.img2img_run_steps``, the truncated loop's indexing against a closed form in float64, ``dpm_step_coefs``'s ``n_nodes``, the argument
checks of ``gl_q_sample``, the three samplers on a recording engine (which timesteps, coefficients and fuser scales a truncated run issues),
and the refusals of the public entries before a model is touched.

The closed form: with the eps oracle of a point-mass data distribution at z0, eps(x, t) = (x - sqrt(acp[t]) z0) / sqrt(1 - acp[t]), a latent of the
form x = sqrt(acp[t]) z0 + sqrt(1 - acp[t]) noise has eps == noise, every sampler's update keeps that form at the step's a_prev, and the loop ends at
sqrt(acp[0]) z0 + sqrt(1 - acp[0]) noise.  A table index that does not belong to its timestep breaks both.  One corner is the reference's own
(plms.py:149): when ONE PLMS node runs, the second evaluation of the double-evaluation step has no next timestep and re-evaluates x_mid --
which already sits at a_prev = acp[0] -- at the same t, so there eps != noise whatever the indexing is; on that step the closed form is
asserted on the first evaluation and on x_mid (the first-order x_prev), and the quirk itself is asserted to be what breaks the rest."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import norel_cases as nc
import stubs
import test_cfg3_host as tch
from layoutllm_t2i_amd import _lib, host, txt2img
from layoutllm_t2i_amd import gligen_inference as gi
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import sampler as sampler_mod
from layoutllm_t2i_amd.arch import TINY
from layoutllm_t2i_amd.model import LatentDiffusion
from layoutllm_t2i_amd.sampler import SAMPLER_KEYS, resolve_sampler

KEY = "strength"
ACP = host.alphas_cumprod()
RUN_STEPS = [((7, 0.5), 3), ((7, 1.0), 7), ((7, 0.1), 1), ((4, 0.5), 2), ((50, 0.75), 37), ((50, 0.8), 40), ((20, 0.3), 6)]


# ------------------------------------------------------------------------------------------- the two host functions
@pytest.mark.parametrize("case,want", RUN_STEPS, ids=[f"{n}-{s}" for (n, s), _ in RUN_STEPS])
def test_run_steps_literal_cases(case, want):
    got = host.img2img_run_steps(*case)
    assert got == want and type(got) is int


def test_check_strength_values():
    for v in (1, 1.0, 0.01, np.float32(0.5)):
        got = host.check_strength(v)
        assert got == float(v) and type(got) is float
    for bad in (0, -0.1, 1.0001, True, float("nan"), float("inf"), "0.5"):
        with pytest.raises(ValueError, match=KEY):
            host.check_strength(bad)
    # the key is no part of the sampler switch
    spec, values = resolve_sampler({KEY: 0.5})
    assert KEY not in SAMPLER_KEYS and KEY not in values and spec.name == "plms"


# ------------------------------------------------------------------------------------------- the truncated loop against the closed form
SCHEDULES = {"plms": lambda: host.make_schedule(6, ACP), "ddim": lambda: host.make_ddim_schedule(6, ACP, "quad", 0),
             "dpmpp_2m": lambda: host.make_dpm_schedule(6, ACP)}
RTOL = 1e-9


def _close(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def truncated_loop(name, sched, strength, z0, noise):
    """the truncated loop of sampler._Sampler restated in float64 on the eps oracle: returns (x, the eps of every evaluation, x_mid or None)"""
    acp = ACP.astype(np.float64)
    form = lambda a: np.sqrt(a) * z0 + np.sqrt(1.0 - a) * noise
    eps_of = lambda x, t: (x - np.sqrt(acp[t]) * z0) / np.sqrt(1.0 - acp[t])
    ts = sched["ddim_timesteps"]
    n = len(ts)
    n_run = host.img2img_run_steps(n, strength)
    time_range = np.flip(ts)[n - n_run:]
    assert len(time_range) == n_run
    x = form(acp[int(time_range[0])])                   # q_sample(z0, t0, noise)
    seen, old, prev, hist, x_mid = [], [], None, None, None
    for i, t in enumerate(time_range):
        index = n_run - i - 1
        a_t, a_prev = float(sched["ddim_alphas"][index]), float(sched["ddim_alphas_prev"][index])

        def x_prev_of(e):
            return np.sqrt(a_prev) * (x - np.sqrt(1.0 - a_t) * e) / np.sqrt(a_t) + np.sqrt(1.0 - a_prev) * e
        e_t = eps_of(x, int(t))
        seen.append(e_t)
        if name == "ddim":
            assert sched["ddim_sigmas"][index] == 0
            x = x_prev_of(e_t)
        elif name == "plms":
            if not old:
                x_mid = x_prev_of(e_t)
                e_next = eps_of(x_mid, int(time_range[min(i + 1, n_run - 1)]))
                seen.append(e_next)
                e_p = (e_t + e_next) / 2
            else:
                coefs, div = host.PLMS_COEFS[min(len(old), 3)]
                e_p = sum(c * e for c, e in zip(coefs, [e_t] + old[::-1])) / div
            x = x_prev_of(e_p)
            old = (old + [e_t])[-3:]
        else:
            h = float(sched["lambdas_prev"][index]) - float(sched["lambdas"][index])
            first = prev is None or (index == 0 and n_run < host.DPM_LOWER_ORDER_FINAL)
            x0 = (x - np.sqrt(1.0 - a_t) * e_t) / np.sqrt(a_t)
            if first:
                d = x0
            else:
                r = (float(sched["lambdas_prev"][prev]) - float(sched["lambdas"][prev])) / h
                d = (1.0 + 1.0 / (2.0 * r)) * x0 - 1.0 / (2.0 * r) * hist
            x = np.sqrt(1.0 - a_prev) / np.sqrt(1.0 - a_t) * x - np.sqrt(a_prev) * np.expm1(-h) * d
            hist, prev = x0, index
    return x, seen, x_mid


@pytest.mark.parametrize("strength", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_truncated_loop_meets_the_closed_form(name, strength):
    sched = SCHEDULES[name]()
    rng = np.random.default_rng(3)
    z0, noise = rng.standard_normal((4, 8, 8)), rng.standard_normal((4, 8, 8))
    end = np.sqrt(np.float64(ACP[0])) * z0 + np.sqrt(1.0 - np.float64(ACP[0])) * noise
    x, seen, x_mid = truncated_loop(name, sched, strength, z0, noise)
    n_run = host.img2img_run_steps(len(sched["ddim_timesteps"]), strength)
    assert len(seen) == n_run + (name == "plms")
    errs = [_close(e, noise) for e in seen]
    print(f"[img2img_closed_form] {name:8s} strength {strength}: {n_run} of {len(sched['ddim_timesteps'])} nodes, max rel |eps - noise| = "
          f"{max(errs):.2e}, rel |x_end - closed form| = {_close(x, end):.2e}")
    if name == "plms" and n_run == 1:
        # plms.py:149 with one node: the second evaluation is x_mid (at a_prev) re-evaluated at the same t -- see the module docstring
        assert errs[0] <= RTOL and _close(x_mid, end) <= RTOL
        assert errs[1] > 1e-3 and _close(x, end) > 1e-6, "the corner is the reference's double evaluation, not the indexing"
        return
    assert max(errs) <= RTOL, errs
    assert _close(x, end) <= RTOL


def test_a_shifted_table_index_breaks_the_closed_form():
    """the point of the closed form: the full schedule's index of a step (n - i - 1 in place of n_run - i - 1) does not belong to its timestep"""
    sched = SCHEDULES["ddim"]()
    n = len(sched["ddim_timesteps"])
    n_run = host.img2img_run_steps(n, 0.5)
    shifted = {k: (v[n - n_run:] if k != "ddim_timesteps" else v) for k, v in sched.items()}
    rng = np.random.default_rng(3)
    z0, noise = rng.standard_normal((4, 8, 8)), rng.standard_normal((4, 8, 8))
    x, seen, _ = truncated_loop("ddim", shifted, 0.5, z0, noise)
    assert max(_close(e, noise) for e in seen) > 1e-3


# ------------------------------------------------------------------------------------------- dpm_step_coefs(n_nodes=)
def test_dpm_step_coefs_counts_the_nodes_that_run():
    import inspect
    assert inspect.signature(host.dpm_step_coefs).parameters["n_nodes"].default is None
    for S in (6, 20):
        sched = host.make_dpm_schedule(S, ACP)
        n = len(sched["ddim_timesteps"])
        assert n == S
        for order in (2, 1):
            for index in range(n):
                for prev in (None, index + 1 if index + 1 < n else None):
                    today = host.dpm_step_coefs(sched, index, prev, order)
                    assert host.dpm_step_coefs(sched, index, prev, order, n_nodes=None) == today
                    assert host.dpm_step_coefs(sched, index, prev, order, n_nodes=n) == today
    sched = host.make_dpm_schedule(20, ACP)
    second = host.dpm_step_coefs(sched, 0, 1, 2)
    assert second[4:] != (1.0, 0.0), "20 nodes: the last step is second order"
    for n_nodes in (1, 6, 14):
        got = host.dpm_step_coefs(sched, 0, 1, 2, n_nodes=n_nodes)
        assert got[4:] == (1.0, 0.0) and got[:4] == second[:4]
    assert host.dpm_step_coefs(sched, 0, 1, 2, n_nodes=15) == second
    assert host.dpm_step_coefs(sched, 3, 4, 2, n_nodes=6) == host.dpm_step_coefs(sched, 3, 4, 2), "only index 0 reads the count"


# ------------------------------------------------------------------------------------------- the C entry, without a GPU
def test_q_sample_is_declared_and_refuses_bad_arguments_without_a_device():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gligen_hip.h")).read()
    assert re.search(r"\bint\s+gl_q_sample\s*\(", header) and "gl_q_sample" in _lib.PROTOTYPES
    lib = _lib.lib()
    assert lib.gl_abi_version() == 15 == _lib.ABI_VERSION
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float))
    for x0, noise, out in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.gl_q_sample(x0, noise, 0.5, 0.5, 1, 4, 1, out, None) == -1
    for B, chw, x0_batch in ((0, 4, 1), (-1, 4, 1), (1, 0, 1), (1, -4, 1), (2, 4, 3), (2, 4, 0), (3, 4, 2)):
        assert lib.gl_q_sample(p, p, 0.5, 0.5, B, chw, x0_batch, p, None) == -1, (B, chw, x0_batch)


# ------------------------------------------------------------------------------------------- the samplers on a recording engine
def _run(monkeypatch, name, cfg, strength=None, init=None, layout=None, mask=False):
    log = []
    tch._ops_spy(monkeypatch, log)
    monkeypatch.setattr(sampler_mod.ops, "q_sample", lambda x0, noise, a, s, out=None: log.append(("q_sample", dict(a=a, s=s, x0=x0, noise=noise))))
    cls, kw, _, _ = tch.SAMPLERS[name]
    model = tch._model(cfg, log)
    inp = tch._inputs(cfg)
    n_alpha = []
    s = cls(LatentDiffusion(), model, alpha_generator_func=lambda n: n_alpha.append(n) or host.alpha_generator(n, tch.ALPHA),
            set_alpha_scale=itf.set_alpha_scale, **kw)
    g = model.grounding_tokenizer_input.prepare(dict(boxes=inp["boxes"], masks=inp["masks"], text_embeddings=inp["positive_embeddings"]), None)
    input = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], relations=inp["relations"], grounding_input=g)
    more = dict(mask=torch.ones(1, 1, 8, 8), x0=torch.zeros(1, 4, 8, 8)) if mask else {}
    shape = tuple(inp["x"].shape)
    torch.manual_seed(11)
    if strength is None:
        s.sample(S=tch.S, shape=shape, input=input, uc=inp["uc"], guidance_scale=tch.G, **more)
    else:
        s.sample_from(tch.S, shape, input, inp["uc"], tch.G, init, strength, layout_guidance_scale=layout, **more)
    return log, torch.get_rng_state(), inp, s, n_alpha


INIT = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 4, 8, 8)).astype(np.float32))
_COEFS = {"plms_step": ("sched",), "ddim_step": ("sqrt_at", "s1m", "sqrt_aprev", "dir_coef", "sigma"), "dpmpp_step": ("sqrt_at", "s1m", "c_x", "c_d")}


@pytest.mark.parametrize("strength", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("name", list(tch.SAMPLERS))
def test_truncated_run_issues_the_tail_of_the_full_run(monkeypatch, name, strength):
    step = tch.SAMPLERS[name][2]
    full, _, _, s_full, _ = _run(monkeypatch, name, nc.NR_TINY)
    log, _, inp, s, n_alpha = _run(monkeypatch, name, nc.NR_TINY, strength=strength, init=INIT)
    ts = [float(t) for t in np.flip(s.ddim_timesteps)]
    n = len(ts)
    n_run = host.img2img_run_steps(n, strength)
    assert n_alpha == [n_run], "the fuser schedule spans the steps that run"
    # the start: one q_sample at the first timestep that runs, on the caller's noise, with the blend's coefficients
    q = [e[1] for e in log if e[0] == "q_sample"]
    ld = LatentDiffusion()
    t0 = int(ts[n - n_run])
    assert len(q) == 1 and q[0]["a"] == float(ld.sqrt_alphas_cumprod[t0]) and q[0]["s"] == float(ld.sqrt_one_minus_alphas_cumprod[t0])
    assert torch.equal(q[0]["x0"], INIT) and torch.equal(q[0]["noise"], inp["x"].float())
    assert [e[0] for e in log][:2] == ["condition", "q_sample"] and not any(e[0] == "q_sample" for e in full)
    # the steps: the timesteps and the schedule scalars of the full run's last n_run nodes, the fuser scales of a schedule of n_run steps
    st, st_full = tch._steps(log)[1:], tch._steps(full)
    assert all(e[0] == step for e in st)
    alphas = host.alpha_generator(n_run, tch.ALPHA)
    ev = list(zip(ts[n - n_run:], alphas))
    if name == "plms":
        ev.insert(1, (ts[n - n_run + 1] if n_run > 1 else ts[-1], alphas[0]))          # the first step that runs evaluates twice
        assert len(st) == n_run + 1 and st[0][1]["coefs"] == (1.0,) and st[1][1]["coefs"] == host.PLMS_COEFS[0][0]
        hist = [e[1]["n_terms"] for e in st[1:]]
        assert hist == [min(max(k + 1, 2), 4) for k in range(n_run)], "the history starts empty at the truncated start"
        tail = st_full[len(st_full) - n_run:]
        assert [e[1]["sched"] for e in st[1:]] == [e[1]["sched"] for e in tail] and st[0][1]["sched"] == st[1][1]["sched"]
    else:
        assert len(st) == n_run
        tail = st_full[n - n_run:]
        for a, b in zip(st, tail):
            assert all(a[1][k] == b[1][k] for k in _COEFS[step]), (a, b)
    assert [(e[1]["t"], e[1]["fuser_scale"]) for e in st] == ev
    if name == "dpmpp_2m":
        assert (st[0][1]["w1"], st[0][1]["w0"]) == (1.0, 0.0), "the first step that runs is first order"
        assert (st[-1][1]["w1"], st[-1][1]["w0"]) == (1.0, 0.0), "fewer than 15 nodes run: the last one is first order"
        assert all(e[1]["w0"] != 0 for e in st[1:-1])


@pytest.mark.parametrize("mask", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("name", list(tch.SAMPLERS))
def test_the_start_draws_nothing(monkeypatch, name, mask):
    """strength 1 runs every node: the torch RNG stream ends where ``sample()`` leaves it"""
    _, plain, _, _, _ = _run(monkeypatch, name, TINY, mask=mask)
    log, keyed, _, _, _ = _run(monkeypatch, name, TINY, strength=1.0, init=INIT, mask=mask)
    assert any(e[0] == "q_sample" for e in log) and torch.equal(plain, keyed)


def test_three_branch_guidance_composes(monkeypatch):
    log, _, _, s, _ = _run(monkeypatch, "ddim", nc.NR_TINY, strength=0.5, init=INIT, layout=12.0)
    n_run = host.img2img_run_steps(len(s.ddim_timesteps), 0.5)
    alphas = host.alpha_generator(n_run, tch.ALPHA)
    n_on = sum(1 for a in alphas if a != 0)
    assert 0 < n_on < n_run
    assert [e[0] for e in log] == ["condition", "q_sample"] + ["cfg3_eval", "ddim_update"] * n_on + ["condition"] + ["ddim_step"] * (n_run - n_on)


def test_sampler_refusals_come_before_the_model_is_touched():
    for name, (cls, kw, _, _) in tch.SAMPLERS.items():
        model = tch._model(TINY, [])
        smp = cls(LatentDiffusion(), model, **kw)
        x = torch.zeros(2, 4, 8, 8)
        call = lambda init, strength: smp.sample_from(tch.S, (2, 4, 8, 8), dict(x=x), None, 1, init, strength)
        with pytest.raises(ValueError, match=KEY):
            call(None, 0.5)
        with pytest.raises(ValueError, match=KEY):
            call(INIT, None)
        for bad in (0, True, 1.5, float("nan")):
            with pytest.raises(ValueError, match=KEY):
                call(INIT, bad)
        for bad in (torch.zeros(3, 4, 8, 8), torch.zeros(1, 4, 8, 16), torch.zeros(1, 3, 8, 8), torch.zeros(4, 8, 8), torch.zeros(1, 4, 8, 8).double()):
            with pytest.raises(ValueError, match="init_latent"):
                call(bad, 0.5)
        assert model.engine.log == []


# ------------------------------------------------------------------------------------------- the public entries
def test_interface_check_strength():
    assert itf.check_strength(None, False) is None
    assert itf.check_strength(None, True) == 0.75 == host.IMG2IMG_DEFAULT_STRENGTH
    assert itf.check_strength(0.3, True) == 0.3 and itf.check_strength(1, True) == 1.0
    with pytest.raises(ValueError, match=KEY):
        itf.check_strength(0.5, False)
    for bad in (0, True, "0.5", 2):
        for has in (True, False):
            with pytest.raises(ValueError, match=KEY):
                itf.check_strength(bad, has)


def test_bad_values_are_refused_at_every_public_entry():
    am = (tch._Untouchable(TINY), None, None, None, {})
    noise = torch.zeros(1, 4, 16, 16)
    meta = dict(prompt="p", phrases=[], locations=[])
    for bad in (0, True, -1.0, float("nan"), "0.5"):
        with pytest.raises(ValueError, match=KEY):
            itf.run_one_image(am, {"batch_size": 1, "guidance_scale": 7.5, KEY: bad}, dict(meta, init_image=object()), noise)
        with pytest.raises(ValueError, match=KEY):
            itf.denoise(am, None, None, None, None, noise, init_latent=torch.zeros(1, 4, 16, 16), strength=bad)
        with pytest.raises(ValueError, match=KEY):
            txt2img.generate(am, None, None, "p", None, None, init_image=object(), strength=bad)
    # the key without an image, and an image's latent without the key
    with pytest.raises(ValueError, match=KEY):
        itf.run_one_image(am, {"batch_size": 1, "guidance_scale": 7.5, KEY: 0.5}, dict(meta), noise)
    with pytest.raises(ValueError, match=KEY):
        itf.run_batch_images(am, {"batch_size": 1, "guidance_scale": 7.5, KEY: 0.5}, dict(prompts=["p"]), noise)
    with pytest.raises(ValueError, match=KEY):
        itf.denoise(am, None, None, None, None, noise, strength=0.5)
    with pytest.raises(ValueError, match=KEY):
        itf.denoise(am, None, None, None, None, noise, init_latent=torch.zeros(1, 4, 16, 16))
    with pytest.raises(ValueError, match=KEY):
        txt2img.generate(am, None, None, "p", None, None, strength=0.5)
    assert am[4] == {}, "refused before the cached config was touched"


def test_public_entries_hand_the_keys_on_per_call(monkeypatch):
    from PIL import Image
    seen, encoded = [], []

    def fake_denoise(all_models, context, uc, relations, batch, noise, *a, **k):
        seen.append(dict(k))
        return noise
    grounding = lambda meta, clip, proc, bs, device=None: dict(boxes=torch.zeros(bs, 30, 4), masks=torch.zeros(bs, 30),
                                                               text_embeddings=torch.zeros(bs, 30, 768))
    monkeypatch.setattr(itf, "denoise", fake_denoise)
    monkeypatch.setattr(itf, "prepare_batch", grounding)
    monkeypatch.setattr(itf, "prepare_batch_multiple", grounding)
    stubs.install_fake_sng_parser()

    class _Vae:
        def encode(self, img):
            encoded.append(tuple(img.shape))
            return torch.randn(img.shape[0], 4, img.shape[2] // 8, img.shape[3] // 8)

        def decode(self, z):
            return torch.zeros(z.shape[0], 3, 4, 4)
    m = type("M", (), {})()
    m.cfg = nc.NR_TINY
    am = (m, _Vae(), stubs.StubTextEncoder(), None, {})
    noise = torch.zeros(2, 4, 16, 24)
    base = dict(batch_size=2, guidance_scale=7.5, no_plms=False)
    meta = dict(prompt="cat sitting on mat", phrases=["cat"], locations=[[0, 0, 1, 1]])
    im = Image.fromarray(np.random.default_rng(0).integers(0, 255, (40, 60, 3), dtype=np.uint8))
    itf.run_one_image(am, dict(base, **{KEY: 0.5}), dict(meta, init_image=im), noise)
    itf.run_one_image(am, dict(base), dict(meta), noise)                          # the cached config still holds the key: the call decides
    itf.run_one_image(am, dict(base), dict(meta, init_image=im), noise)           # ... and does not supply it either: the default
    itf.run_one_image(am, dict(base, **{KEY: None}), dict(meta, init_image=im), noise)
    assert seen[0][KEY] == 0.5 and tuple(seen[0]["init_latent"].shape) == (1, 4, 16, 24) and encoded[0] == (1, 3, 128, 192)
    assert KEY not in seen[1] and "init_latent" not in seen[1], "without the keys denoise is called as it always was"
    assert seen[2][KEY] == 0.75 == seen[3][KEY]
    bmeta = dict(prompts=[meta["prompt"]] * 2, phrases=[["cat"]] * 2, locations=[[[0, 0, 1, 1]]] * 2)
    itf.run_batch_images(am, dict(base, sampler="ddim", **{KEY: 1}), dict(bmeta, init_image=[im, im]), noise)
    assert seen[4][KEY] == 1.0 and seen[4]["sampler"] == "ddim" and tuple(seen[4]["init_latent"].shape) == (2, 4, 16, 24)
    n_enc = len(encoded)
    with pytest.raises(ValueError, match="init_image"):
        itf.run_batch_images(am, dict(base), dict(bmeta, init_image=[im, im, im]), noise)
    assert len(encoded) == n_enc and len(seen) == 5, "a list of the wrong length is refused before any encoder runs"
    # together with inpainting: input_image is encoded first, then init_image; both reach denoise
    itf.run_one_image(am, dict(base, **{KEY: 0.5}), dict(meta, init_image=im, input_image=im), noise)
    assert len(encoded) == n_enc + 2 and seen[5]["mask"] is not None and seen[5]["x0"] is not None and seen[5][KEY] == 0.5
    # gligen_inference.run takes both keys in its config and forwards them when present, and only then
    got = []
    monkeypatch.setattr(itf, "run_one_image", lambda am_, args, m_, noise_, clip, proc, device=None: got.append((dict(args), dict(m_))) or [])
    monkeypatch.setitem(gi._MODELS, "ck", (type("M", (), {"first_conv_type": "SD"})(), None, None, None, {}))
    gmeta = dict(ckpt="ck", prompt="p", phrases=["a"], locations=[[0, 0, 1, 1]])
    gi.run(gmeta, {"batch_size": 1, "device": "cpu", KEY: 0.4, "init_image": im}, noise[:1], clip_model=object(), clip_processor=object())
    gi.run(gmeta, dict(batch_size=1, device="cpu"), noise[:1], clip_model=object(), clip_processor=object())
    assert got[0][0][KEY] == 0.4 and got[0][1]["init_image"] is im
    assert KEY not in got[1][0] and "init_image" not in got[1][1]
