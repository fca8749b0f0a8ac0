"""The host side of the DDIM sampler, without a GPU: the schedule tables and step scalars against the reference's (bit for bit, dtypes
included), tests/ddim_ref.py against the latents of the reference's own DDIMSampler with its noise draws replayed, and the argument
handling of the public switch with the engine stubbed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ddim_cases as dc
import ddim_ref
import norel_cases as nc
import norel_ref
import stubs
import test_oracle_golden as tog
from layoutllm_t2i_amd import gligen_inference as gi
from layoutllm_t2i_amd import host, recipe, txt2img
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY
from layoutllm_t2i_amd.model import LatentDiffusion
from layoutllm_t2i_amd.sampler import DDIMSampler, PLMSSampler

GOLD = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
DENOISE = itf.denoise            # the real one: the run_spy fixture replaces the module attribute
DTYPES = dict(ddim_timesteps=np.int64, ddim_alphas=np.float32, ddim_alphas_prev=np.float64, ddim_sqrt_one_minus_alphas=np.float32,
              ddim_sigmas=np.float64)


# ------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("S,disc,eta", dc.SCHEDULE_CASES, ids=[dc.schedule_tag(*c) for c in dc.SCHEDULE_CASES])
def test_schedule_and_step_scalars_equal_the_reference_bit_for_bit(S, disc, eta):
    g = np.load(os.path.join(GOLD, "ddim_schedule.npz"))
    tag = dc.schedule_tag(S, disc, eta)
    s = host.make_ddim_schedule(S, host.alphas_cumprod(), disc, eta)
    for k in dc.SCHEDULE_KEYS:
        ref = g[f"{tag}.{k}"]
        assert ref.dtype == DTYPES[k], (k, ref.dtype)                    # the reference's dtypes, as the issue lists them
        assert s[k].dtype == ref.dtype and s[k].shape == ref.shape, (k, s[k].dtype, s[k].shape)
        assert s[k].tobytes() == ref.tobytes(), k
    coefs = np.asarray([host.ddim_step_coefs(s, i) for i in range(len(s["ddim_timesteps"]))], np.float32)
    assert coefs.tobytes() == g[f"{tag}.coefs"].tobytes()
    assert np.isfinite(coefs).all()
    if (S, disc) == (6, "uniform"):
        assert len(s["ddim_timesteps"]) == 7                             # range(0, 1000, 1000 // 6)
    if (S, disc) == (50, "quad"):
        assert len(set(s["ddim_timesteps"].tolist())) < 50               # quad repeats timesteps at its low end
    if eta == 0:
        assert not s["ddim_sigmas"].any()
        # with eta 0 the four PLMS scalars are the DDIM ones
        plms = host.make_schedule(S, host.alphas_cumprod())
        assert all(host.step_coefs(plms, i) == host.ddim_step_coefs(s, i)[:4] for i in range(len(s["ddim_timesteps"])))
    else:
        # a repeated timestep has a_t == a_prev, hence sigma 0 (a step that changes nothing); every other step is stochastic
        repeated = np.concatenate([[False], np.diff(s["ddim_timesteps"]) == 0])
        assert ((s["ddim_sigmas"] == 0) == repeated).all()


def test_schedule_refuses_bad_arguments():
    acp = host.alphas_cumprod()
    with pytest.raises(ValueError, match="ddim_discretize"):
        host.make_ddim_schedule(10, acp, "cosine")
    for eta in (-0.1, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="ddim_eta"):
            host.make_ddim_schedule(10, acp, "uniform", eta)


# ------------------------------------------------------------------------------------------- the restated loop against the reference's runs
def _eps_fn(case, inp):
    if case["unet"] == "norel":
        sd = {k: T(np.asarray(v)) for k, v in recipe.state_dict(nc.NR_TINY, 0).items()}
        fc = {a: T(v) for a, v in recipe.sd_first_conv(nc.NR_TINY, 0).items()}
        return norel_ref.make_eps_fn(sd, nc.NR_TINY, inp, case["guidance"], fc)
    return tog.make_eps_fn(case, inp, tog.tiny_sd(), TINY)


@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_ddim_ref_matches_the_reference_sampler(case):
    """the bound of tests/test_oracle_golden.py::test_plms_tiny_matches_reference; every draw of the reference run is replayed, in its order
    and shape (q_sample's draw on x0 first, the latent's draw on every step, sigma 0 included)"""
    g = np.load(os.path.join(GOLD, case["name"] + ".npz"))
    inp = {a: T(v) for a, v in dc.case_inputs(case).items()}
    sched = host.make_ddim_schedule(case["S"], host.alphas_cumprod(), case["discretize"], case["eta"])
    assert np.array_equal(sched["ddim_timesteps"], g["ddim_timesteps"])
    draws = dc.unpack_draws(g)
    steps = len(sched["ddim_timesteps"])
    assert len(draws) == steps * (2 if case["mask"] else 1)
    fake, state = dc.replayer(draws)
    with torch.no_grad(), dc.patched_randn_like(fake):
        out = ddim_ref.ddim_sample(_eps_fn(case, inp), inp["x"], sched, case["alpha_type"], mask=inp.get("mask"), x0=inp.get("x0"))
    assert state["n"] == len(draws)
    ref = g["out"]
    err = np.abs(out.numpy() - ref).max() / np.abs(ref).max()
    print(f"[{case['name']}] max-abs / max = {err:.3e}")
    assert err < 2e-4, err


def test_goldens_depend_on_eta():
    """the fixtures are not degenerate: the reference's eta 1 latent is far from its eta 0 latent, so replaying the draws is a real test"""
    a, b = (np.load(os.path.join(GOLD, n + ".npz"))["out"] for n in ("ddim_norel_eta0", "ddim_norel_eta1"))
    assert np.linalg.norm(a - b) / np.linalg.norm(a) > 0.1


# ------------------------------------------------------------------------------------------- argument handling, engine stubbed
class _Decoder:
    def decode(self, z):
        return torch.zeros(z.shape[0], 3, 4, 4)


@pytest.fixture()
def run_spy(monkeypatch):
    seen = []

    def fake_denoise(all_models, context, uc, relations, batch, noise, *a, **k):
        seen.append({n: k.get(n, "absent") for n in ("sampler", "ddim_eta", "ddim_discretize", "steps")})
        return noise
    grounding = lambda meta, clip, proc, bs, device=None: dict(boxes=torch.zeros(bs, 30, 4), masks=torch.zeros(bs, 30),
                                                               text_embeddings=torch.zeros(bs, 30, 768))
    monkeypatch.setattr(itf, "denoise", fake_denoise)
    monkeypatch.setattr(itf, "prepare_batch", grounding)
    monkeypatch.setattr(itf, "prepare_batch_multiple", grounding)
    stubs.install_fake_sng_parser()
    return seen


def _all_models():
    m = type("M", (), {})()
    m.cfg = nc.NR_TINY
    return (m, _Decoder(), stubs.StubTextEncoder(), None, {})


META = dict(prompt="cat sitting on mat", phrases=["cat"], locations=[[0, 0, 1, 1]])
BAD_ARGS = [
    (dict(sampler="euler"), "sampler"),
    (dict(sampler="DDIM"), "sampler"),
    (dict(sampler="ddim", ddim_eta=-0.5), "ddim_eta"),
    (dict(sampler="ddim", ddim_eta=float("nan")), "ddim_eta"),
    (dict(sampler="ddim", ddim_eta=float("inf")), "ddim_eta"),
    (dict(sampler="ddim", ddim_discretize="cosine"), "ddim_discretize"),
    (dict(sampler="plms", ddim_eta=0.5), "plms"),
    (dict(ddim_eta=0.5), "plms"),                                        # the default sampler is PLMS
    (dict(ddim_discretize="quad"), "plms"),
]


@pytest.mark.parametrize("more,match", BAD_ARGS, ids=[str(i) for i in range(len(BAD_ARGS))])
def test_bad_sampler_arguments_raise_before_anything_runs(run_spy, more, match):
    am = _all_models()
    noise = torch.zeros(2, 4, 16, 16)
    with pytest.raises(ValueError, match=match):
        itf.run_one_image(am, dict(batch_size=2, guidance_scale=7.5, no_plms=False, **more), dict(META), noise)
    assert not run_spy and "sampler" not in am[4], "refused before the config was touched and before denoise ran"
    with pytest.raises(ValueError, match=match):
        DENOISE((None, None, None, None, {}), None, None, None, None, noise, **more)      # denoise itself checks first, too


def test_sampler_keys_are_read_per_call_and_are_not_sticky(run_spy):
    am = _all_models()
    noise = torch.zeros(2, 4, 16, 16)
    base = dict(batch_size=2, guidance_scale=7.5, no_plms=False)
    itf.run_one_image(am, dict(base, sampler="ddim", ddim_eta=0.5, ddim_discretize="quad", steps=4), dict(META), noise)
    itf.run_one_image(am, dict(base), dict(META), noise)                 # the cached config still holds "ddim": the call decides
    itf.run_batch_images(am, dict(base, sampler="ddim"), dict(prompts=[META["prompt"]] * 2, phrases=[["cat"]] * 2,
                                                               locations=[[[0, 0, 1, 1]]] * 2), noise)
    assert run_spy[0] == dict(sampler="ddim", ddim_eta=0.5, ddim_discretize="quad", steps=4)
    assert run_spy[1] == dict(sampler="plms", ddim_eta=0.0, ddim_discretize="uniform", steps=itf.PLMS_STEPS)
    assert run_spy[2] == dict(sampler="ddim", ddim_eta=0.0, ddim_discretize="uniform", steps=itf.PLMS_STEPS)


def test_no_plms_still_raises_and_points_at_the_switch(run_spy):
    with pytest.raises(NotImplementedError, match=r'args\["sampler"\] = "ddim"'):
        itf.run_one_image(_all_models(), dict(batch_size=2, guidance_scale=7.5, no_plms=True), dict(META), torch.zeros(2, 4, 16, 16))
    with pytest.raises(NotImplementedError):
        itf.run_one_image(_all_models(), dict(batch_size=2, guidance_scale=7.5, no_plms=True, sampler="ddim"), dict(META), torch.zeros(2, 4, 16, 16))
    assert not run_spy


def test_gligen_inference_run_hands_the_sampler_keys_on(monkeypatch):
    seen = []
    monkeypatch.setattr(itf, "run_one_image", lambda am, args, m, noise, clip, proc, device=None: seen.append(dict(args)) or [])
    monkeypatch.setitem(gi._MODELS, "ck", (type("M", (), {"first_conv_type": "SD"})(), None, None, None, {}))
    meta = dict(ckpt="ck", prompt="p", phrases=["a"], locations=[[0, 0, 1, 1]])
    noise = torch.zeros(1, 4, 16, 16)
    gi.run(meta, dict(batch_size=1, device="cpu", sampler="ddim", ddim_eta=0.5, ddim_discretize="quad", steps=4), noise, clip_model=object(),
           clip_processor=object())
    gi.run(meta, dict(batch_size=1, device="cpu"), noise, clip_model=object(), clip_processor=object())
    assert (seen[0]["sampler"], seen[0]["ddim_eta"], seen[0]["ddim_discretize"], seen[0]["steps"]) == ("ddim", 0.5, "quad", 4)
    assert not {"sampler", "ddim_eta", "ddim_discretize", "steps"} & set(seen[1])


def test_txt2img_generate_checks_the_sampler_first():
    class _M:
        cfg = TINY
    with pytest.raises(ValueError, match="sampler"):
        txt2img.generate((_M(), None, None, None, {}), None, None, "p", None, None, sampler="euler")
    with pytest.raises(ValueError, match="ddim_eta"):
        txt2img.generate((_M(), None, None, None, {}), None, None, "p", None, None, sampler="ddim", ddim_eta=-1.0)
    with pytest.raises(ValueError, match="plms"):
        txt2img.generate((_M(), None, None, None, {}), None, None, "p", None, None, ddim_eta=0.5)


# ------------------------------------------------------------------------------------------- the sampler class, engine stubbed
class _StubEngine:
    def __init__(self):
        self.steps = []

    def buf(self, tag, shape, dtype=torch.float32, zero=False):
        return torch.zeros(tuple(shape), dtype=dtype)

    def ddim_step(self, x, x_out, **kw):
        self.steps.append(kw)
        return x_out


class _StubModel:
    device = "cpu"
    fuser_scale = 1.0
    use_sd_conv = False

    def __init__(self):
        self.engine = _StubEngine()

    def condition(self, input, uc, always_extra=False):
        return 1 if uc is None else 2


def test_sample_keeps_the_constructors_eta_and_discretisation():
    """unlike the reference's sample(), which re-makes the schedule with eta 0 on uniform steps"""
    m = _StubModel()
    s = DDIMSampler(LatentDiffusion(), m, eta=0.5, discretize="quad")
    x = torch.zeros(2, 4, 16, 16)
    draws = []
    real = torch.randn_like
    with dc.patched_randn_like(lambda t, *a, **k: draws.append(tuple(t.shape)) or real(t)):
        s.sample(S=8, shape=tuple(x.shape), input=dict(x=x), uc=torch.zeros(2, 77, 768), guidance_scale=7.5)
    want = host.make_ddim_schedule(8, host.alphas_cumprod(), "quad", 0.5)
    assert np.array_equal(s.ddim_timesteps, want["ddim_timesteps"]) and s.ddim_sigmas.tobytes() == want["ddim_sigmas"].tobytes()
    steps = m.engine.steps
    assert len(steps) == 8 and all(k["reps"] == 2 and k["noise"] is not None for k in steps)
    assert [k["sigma"] for k in steps] == [host.ddim_step_coefs(want, i)[4] for i in range(7, -1, -1)] and all(k["sigma"] > 0 for k in steps)
    assert [k["t"] for k in steps] == [float(t) for t in want["ddim_timesteps"][::-1]]
    assert draws == [(2, 4, 16, 16)] * 8
    # eta 0: the draw is still made on every step (ddim.py:132), and the kernel gets no noise
    m0 = _StubModel()
    draws.clear()
    with dc.patched_randn_like(lambda t, *a, **k: draws.append(tuple(t.shape)) or real(t)):
        DDIMSampler(LatentDiffusion(), m0).sample(S=6, shape=tuple(x.shape), input=dict(x=x), uc=None, guidance_scale=7.5)
    assert len(m0.engine.steps) == 7 and all(k["noise"] is None and k["sigma"] == 0 and k["reps"] == 1 for k in m0.engine.steps)
    assert draws == [(2, 4, 16, 16)] * 7


def test_sampler_constructor_and_make_schedule_arguments():
    m = _StubModel()
    with pytest.raises(ValueError, match="ddim_eta"):
        DDIMSampler(LatentDiffusion(), m, eta=-1.0)
    with pytest.raises(ValueError, match="ddim_discretize"):
        DDIMSampler(LatentDiffusion(), m, discretize="cosine")
    s = DDIMSampler(LatentDiffusion(), m)
    s.make_schedule(10, ddim_discretize="uniform", ddim_eta=1.0)         # the reference's route to eta: make_schedule + ddim_sampling
    assert (s.ddim_sigmas > 0).all() and s.ddim_alphas.dtype == np.float32 and s.ddim_alphas_prev.dtype == np.float64
    # PLMS keeps refusing both
    p = PLMSSampler(LatentDiffusion(), m)
    with pytest.raises(ValueError):
        p.make_schedule(10, ddim_eta=0.5)
    with pytest.raises(NotImplementedError):
        p.make_schedule(10, ddim_discretize="quad")


def test_plms_sampler_calls_plms_step_by_position():
    """``UNetEngine.plms_step`` takes every argument by position, and callers that time it wrap it with exactly that signature (the
    benchmark does): the sampler must not hand any of them over by keyword."""
    calls = []

    class _E(_StubEngine):
        def plms_step(self, x_eval, x_base, x_out, e_out, e_terms, coefs, div, t, reps, guidance, fuser_scale, sd_conv, *sched):
            calls.append((t, reps, guidance, fuser_scale, sd_conv, sched))
            return x_out

    m = _StubModel()
    m.engine = _E()
    x = torch.zeros(2, 4, 16, 16)
    PLMSSampler(LatentDiffusion(), m).sample(S=4, shape=tuple(x.shape), input=dict(x=x), uc=torch.zeros(2, 77, 768), guidance_scale=7.5)
    sched = host.make_schedule(4, host.alphas_cumprod())
    ts = [float(t) for t in sched["ddim_timesteps"][::-1]]
    assert len(calls) == 5                                                        # step 0 evaluates twice
    assert [c[0] for c in calls] == [ts[0], ts[1]] + ts[1:]
    assert all(c[1:5] == (2, 7.5, 1.0, False) for c in calls)
    assert [c[5] for c in calls] == [tuple(host.step_coefs(sched, i)) for i in (3, 3, 2, 1, 0)]
