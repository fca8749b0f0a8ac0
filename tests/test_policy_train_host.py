"""Policy training, host side (no GPU): the C ABI of gl_policy_grad / gl_policy_adam_step and their refusals, PolicyTrainer's checks, its
checkpoint layout against torch's own Adam and StepLR, the golden file against the regenerated cases, and train_batch's host logic
with the trainer replaced by a recorder."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import policy_train_cases as tc
from layoutllm_t2i_amd import _lib, policy_train, prompting, train_rl
from layoutllm_t2i_amd.policy import CandidatePool, PolicyNetwork, sample_examples
from layoutllm_t2i_amd.policy_train import PolicyTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "policy_train_ref.npz"))


def _built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)
    return _lib.lib()


def _aligned():
    dev = (ctypes.c_double * 8)()                       # stands for device memory; refusals never dereference it
    return dev, (ctypes.addressof(dev) + 15) // 16 * 16


# ------------------------------------------------------------------------------------------- C ABI
def test_policy_train_entries_are_exported_under_abi_15():
    l = _built()
    assert l.gl_abi_version() == _lib.ABI_VERSION == 15
    assert l.gl_sizeof_policy_grad_args() == ctypes.sizeof(_lib.PolicyGradArgs) == 128
    assert l.gl_sizeof_policy_adam_args() == ctypes.sizeof(_lib.PolicyAdamArgs) == 112
    assert l.gl_sizeof_policy_args() == ctypes.sizeof(_lib.PolicyArgs) == 104
    hdr = open(os.path.join(ROOT, "include", "gligen_hip.h")).read()
    for fn in ("gl_policy_grad", "gl_sizeof_policy_grad_args", "gl_policy_grad_scratch_bytes", "gl_policy_adam_step", "gl_sizeof_policy_adam_args"):
        assert fn in _lib.PROTOTYPES and hasattr(l, fn) and f" {fn}(" in hdr, fn
    assert "#define GL_POLICY_TRAIN_MAX_CANDS 4096" in hdr and policy_train.MAX_TRAIN_CANDS == 4096
    assert "policy_train.hip" in __import__("layoutllm_t2i_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


def test_policy_grad_scratch_size():
    l = _built()
    a256 = lambda b: (b + 255) // 256 * 256
    for P, N, D, E, k in ((1, 1, 4, 1, 1), (3, 65, 768, 128, 2), (64, 4096, 1024, 1024, 32), (8, 32, 512, 100, 8)):
        assert l.gl_policy_grad_scratch_bytes(P, N, D, E, k) == 2 * a256((P + N) * E * 8) + a256(P * N * 8)
    for bad in ((0, 1, 4, 4, 1), (65, 1, 4, 4, 1), (1, 0, 4, 4, 1), (1, 4097, 4, 4, 1), (1, 1, 0, 4, 1), (1, 1, 6, 4, 1), (1, 1, 1028, 4, 1),
                (1, 1, 4, 0, 1), (1, 1, 4, 1025, 1), (1, 1, 4, 4, 0), (1, 1, 4, 4, 33)):
        assert l.gl_policy_grad_scratch_bytes(*bad) == -1, bad


def test_policy_grad_refuses_bad_arguments_before_any_launch():
    """every refusal is decided on the host from the struct: nothing is launched, so this runs without a GPU"""
    l = _built()
    dev, p = _aligned()

    def args(**kw):
        a = _lib.PolicyGradArgs()
        a.prompt = a.cand = a.W = a.bias = a.sel = a.reward = a.loss = a.logp = a.grad_W = a.grad_b = a.scratch = p
        a.P, a.N, a.D, a.E, a.k, a.temperature, a.scratch_bytes = 3, 65, 768, 128, 2, 1.0, 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(what, **kw):
        assert l.gl_policy_grad(ctypes.byref(args(**kw)), None) == -1, kw
        msg = _lib.last_error(None)
        assert msg.startswith("gl_policy_grad:") and what in msg, (kw, msg)

    assert l.gl_policy_grad(None, None) == -1 and "null args" in _lib.last_error(None)
    for field in ("prompt", "cand", "W", "bias", "sel", "reward", "loss", "logp", "grad_W", "grad_b", "scratch"):
        refused("null", **{field: None})
    refused("nothing to train", W=None)
    refused("P = 0", P=0)
    refused("P = 65", P=65)
    refused("N = 0", N=0)
    refused("N = 4097", N=4097)
    for D in (0, 2, 766, 1028, -4):
        refused(f"D = {D}", D=D)
    refused("E = 0", E=0)
    refused("E = 1025", E=1025)
    refused("k = 0", k=0)
    refused("k = 33", k=33)
    for t in (0.0, -1.0, float("nan")):
        refused("temperature", temperature=t)
    need = l.gl_policy_grad_scratch_bytes(3, 65, 768, 128, 2)
    refused(f"needs {need}", scratch_bytes=need - 1)
    for field in ("prompt", "cand", "W", "scratch"):
        refused("16-byte aligned", **{field: p + 4})
    # the largest sizes are allowed: refused only further on, for the scratch
    refused("scratch of 0 bytes", P=64, N=4096, D=1024, E=1024, k=32, scratch_bytes=0)


def test_policy_adam_step_refuses_bad_arguments_before_any_launch():
    l = _built()
    dev, p = _aligned()

    def args(**kw):
        a = _lib.PolicyAdamArgs()
        a.W = a.bias = a.grad_W = a.grad_b = a.exp_avg_W = a.exp_avg_sq_W = a.exp_avg_b = a.exp_avg_sq_b = p
        a.D, a.E, a.step, a.lr, a.beta1, a.beta2, a.eps = 768, 128, 1, 1e-3, 0.9, 0.999, 1e-8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(what, **kw):
        assert l.gl_policy_adam_step(ctypes.byref(args(**kw)), None) == -1, kw
        msg = _lib.last_error(None)
        assert msg.startswith("gl_policy_adam_step:") and what in msg, (kw, msg)

    assert l.gl_policy_adam_step(None, None) == -1 and "null args" in _lib.last_error(None)
    for field in ("W", "bias", "grad_W", "grad_b", "exp_avg_W", "exp_avg_sq_W", "exp_avg_b", "exp_avg_sq_b"):
        refused("null", **{field: None})
    for D in (0, 2, 1028):
        refused(f"D = {D}", D=D)
    refused("E = 0", E=0)
    refused("E = 1025", E=1025)
    refused("step = 0", step=0)
    refused("step = -2", step=-2)
    for v in (-1e-3, float("nan"), float("inf")):
        refused("lr", lr=v)
        refused("eps", eps=v)
    for v in (-0.1, 1.0, float("nan")):
        refused("beta1", beta1=v)
        refused("beta2", beta2=v)
    # a policy-select refusal shares the calling thread's message slot
    assert l.gl_policy_select(None, None) == -1 and _lib.last_error(None).startswith("gl_policy_select:")


# ------------------------------------------------------------------------------------------- PolicyTrainer
def _net(D=768, E=128):
    return PolicyNetwork(D, E, device="cpu").load_state_dict({"weight": torch.zeros(E, D), "bias": torch.zeros(E)})


def test_policy_trainer_checks_before_a_device_is_needed():
    with pytest.raises(ValueError, match="add_linear=False"):
        PolicyTrainer(PolicyNetwork(add_linear=False, device="cpu"))
    with pytest.raises(ValueError, match="load_state_dict first"):
        PolicyTrainer(PolicyNetwork(device="cpu"))
    tr = PolicyTrainer(_net())
    x, y = torch.zeros(3, 768), torch.zeros(5, 768)
    sel, r = np.zeros((3, 2), np.int64), torch.zeros(3)
    for fn in (tr.loss_and_grad, tr.step):
        with pytest.raises(ValueError, match="65 prompts"):
            fn(torch.zeros(65, 768), y, np.zeros((65, 2), int), torch.zeros(65))
        with pytest.raises(ValueError, match="4097 candidates"):
            fn(x, torch.zeros(4097, 768), sel, r)
        with pytest.raises(ValueError, match="emb_cand"):
            fn(x, torch.zeros(5, 512), sel, r)
        for bad in (np.zeros((2, 2), int), np.zeros(3, int), np.zeros((3, 33), int), np.zeros((3, 0), int), np.zeros((3, 2))):
            with pytest.raises(ValueError, match="sel"):
                fn(x, y, bad, r)
        for bad in (torch.zeros(2), torch.zeros(3, 1), torch.zeros(3, dtype=torch.int64)):
            with pytest.raises(ValueError, match="reward"):
                fn(x, y, sel, bad)
        with pytest.raises(ValueError, match="temperature"):
            fn(x, y, sel, r, 0.0)
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(x, y, sel, r)
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(x, y, torch.zeros(3, 2, dtype=torch.int32), r.double().numpy())
    assert tr.steps == 0


def _torch_pair(lr=1e-3, step_size=20, gamma=0.5, E=6, D=8):
    lin = torch.nn.Linear(D, E)
    opt = torch.optim.Adam(lin.parameters(), lr=lr)
    return lin, opt, torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=gamma)


def _same_structure(a, b, path=""):
    assert type(a) is type(b) or (isinstance(a, (int, float)) and isinstance(b, (int, float))), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), (path, list(a), list(b))
        for k in a:
            _same_structure(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_structure(x, y, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, (path, a.shape, b.shape, a.dtype, b.dtype)


def test_state_dict_has_the_layout_of_torch_adam_and_steplr(tmp_path):
    D, E = 8, 6
    lin, opt, sched = _torch_pair(E=E, D=D)
    tr = PolicyTrainer(PolicyNetwork(D, E, device="cpu").load_state_dict(lin.state_dict()))
    # before any step: torch's state is empty, so is ours
    want = {"optimizer": opt.state_dict(), "lr_scheduler": sched.state_dict()}
    got = tr.state_dict()
    _same_structure(got, want)
    assert got["optimizer"]["state"] == {} and got["optimizer"]["param_groups"] == want["optimizer"]["param_groups"]
    assert got["lr_scheduler"] == want["lr_scheduler"]
    # after steps and epochs (the state set by hand: the step itself runs on the GPU only)
    for _ in range(3):
        lin(torch.randn(4, D)).pow(2).sum().backward()
        opt.step()
        opt.zero_grad()
    for _ in range(23):
        sched.step()
    tr.steps = 3
    tr.exp_avg = [opt.state[p]["exp_avg"].clone() for p in lin.parameters()]
    tr.exp_avg_sq = [opt.state[p]["exp_avg_sq"].clone() for p in lin.parameters()]
    for _ in range(23):
        tr.epoch_end()
    want = {"optimizer": opt.state_dict(), "lr_scheduler": sched.state_dict()}
    got = tr.state_dict()
    _same_structure(got, want)
    assert got["optimizer"]["param_groups"] == want["optimizer"]["param_groups"] and got["lr_scheduler"] == want["lr_scheduler"]
    assert got["optimizer"]["param_groups"][0]["lr"] == 0.5e-3
    for i in (0, 1):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(got["optimizer"]["state"][i][k], want["optimizer"]["state"][i][k]), (i, k)
    # through a file, into a fresh trainer and into a fresh torch optimiser
    path = str(tmp_path / "state_7.pt")
    torch.save(got, path)
    back = torch.load(path, weights_only=True)
    tr2 = PolicyTrainer(PolicyNetwork(D, E, device="cpu").load_state_dict(lin.state_dict()), lr=5.0).load_state_dict(back)
    assert (tr2.steps, tr2.epochs, tr2.lr, tr2.base_lr, tr2.lr_step_size, tr2.lr_gamma) == (3, 23, 0.5e-3, 1e-3, 20, 0.5)
    assert torch.equal(tr2.exp_avg[0], tr.exp_avg[0]) and torch.equal(tr2.exp_avg_sq[1], tr.exp_avg_sq[1])
    _same_structure(tr2.state_dict(), got)
    lin3, opt3, sched3 = _torch_pair(E=E, D=D)
    opt3.load_state_dict(back["optimizer"])
    sched3.load_state_dict(back["lr_scheduler"])
    assert opt3.param_groups[0]["lr"] == 0.5e-3 and sched3.last_epoch == 23
    assert float(opt3.state[lin3.weight]["step"]) == 3 and torch.equal(opt3.state[lin3.bias]["exp_avg"], tr.exp_avg[1])
    # the reference's resume loads the optimiser alone
    tr4 = PolicyTrainer(PolicyNetwork(D, E, device="cpu").load_state_dict(lin.state_dict())).load_state_dict({"optimizer": back["optimizer"]})
    assert (tr4.steps, tr4.lr, tr4.epochs) == (3, 0.5e-3, 0)
    tr4.set_lr(2e-3)
    assert (tr4.lr, tr4.base_lr, tr4.epochs, tr4.steps) == (2e-3, 2e-3, 0, 3)
    for bad in ({}, {"optimizer": {"state": {}, "param_groups": []}},
                {"optimizer": {"state": {0: back["optimizer"]["state"][0]}, "param_groups": back["optimizer"]["param_groups"]}}):
        with pytest.raises(ValueError):
            tr4.load_state_dict(bad)
    assert set(tr.weights()) == {"weight", "bias"} and torch.equal(tr.weights()["weight"], lin.weight.detach())


@pytest.mark.parametrize("step_size,gamma", [(20, 0.5), (7, 0.5), (1, 0.25), (20, 0.9)])
def test_epoch_end_is_steplr(step_size, gamma):
    lin, opt, sched = _torch_pair(lr=1e-3, step_size=step_size, gamma=gamma)
    tr = PolicyTrainer(_net(8, 6), lr=1e-3, lr_step_size=step_size, lr_gamma=gamma)
    for epoch in range(45):
        opt.step()
        sched.step()
        got = tr.epoch_end()
        want = opt.param_groups[0]["lr"]
        # StepLR multiplies the running value, epoch_end takes the power: equal for a gamma that is a power of two, one rounding apart otherwise
        assert got == want if gamma in (0.5, 0.25) else got == pytest.approx(want, rel=1e-13), (epoch, got, want)
        assert tr.state_dict()["lr_scheduler"]["last_epoch"] == sched.last_epoch == epoch + 1


# ------------------------------------------------------------------------------------------- cases and goldens
def test_policy_train_golden_file_matches_the_regenerated_cases():
    names = GOLD["names"].tolist()
    assert names == [tc.case_name(c) for c in tc.CASES] and 36 <= len(tc.CASES) <= 44 and len(set(names)) == len(names)
    assert {tc.CONFIGS[c[0]] for c in tc.CASES} == {(768, 128), (512, 100), (4, 1)}
    assert {c[1] for c in tc.CASES} >= {32, 63, 65, 257} and any(c[1] == c[3] for c in tc.CASES)
    assert {c[2] for c in tc.CASES} == {1, 3, 8, 64} and {c[3] for c in tc.CASES} == {1, 2, 8, 32} and {c[4] for c in tc.CASES} == {0.5, 1.0, 2.0}
    for config in tc.CONFIGS:
        assert {c[1] for c in tc.CASES if c[0] == config} >= {32, 63, 65, 257} and any(c[1] == c[3] for c in tc.CASES if c[0] == config)
    assert GOLD["e_ref"].shape == (len(names), len(tc.OUTPUTS) + len(tc.CHAINED)) and (GOLD["e_ref"] > 0).all()
    for i, case in enumerate(tc.CASES):
        sel, reward = GOLD[names[i] + ".sel"], GOLD[names[i] + ".reward"]
        N, P, k = case[1:4]
        assert sel.shape == (tc.STEPS, P, k) and sel.dtype == np.int32 and sel.min() >= 0 and sel.max() < N
        assert all(len(set(row.tolist())) == k for step in sel for row in step)                 # drawn without replacement
        assert np.array_equal(reward, tc.rewards(case, int(GOLD["seeds"][i])))
        if P >= 3:
            assert (reward[:, 0] > 0).all() and (reward[:, 1] == 0).all() and (reward[:, 2] < 0).all()
    # the generation-time conditions again, for a few named cases
    for name in ("d768_e128_n32_p8_k2_t0.5", "d4_e1_n32_p3_k2_t0.5", "d512_e100_n63_p64_k1_t1", "d768_e128_n2_p1_k2_t0.5"):
        i = names.index(name)
        case, seed = tc.CASES[i], int(GOLD["seeds"][i])
        W, b = tc.layer(case[0])
        prompt, cand = tc.inputs(case, seed)
        assert tc.checksum(prompt, cand) == pytest.approx(GOLD["checksum"][i], rel=1e-12)
        rng = np.random.RandomState(seed)
        draw = lambda probs: np.stack([sample_examples(row, case[3], rng)[::-1] for row in probs])
        r32 = tc.run_torch(W, b, prompt, cand, tc.rewards(case, seed), case[4], torch.float32, draw=draw)
        assert np.array_equal(np.stack(r32["sel"]), GOLD[name + ".sel"])                        # the selections are sample_examples' own
        assert r32["min_sel_prob"] >= tc.MIN_PROB
        r64 = tc.ref64(case, seed, GOLD[name + ".sel"])
        assert r64["loss"][0] == pytest.approx(GOLD["loss64"][i], rel=1e-12)
        err = [float(np.abs(np.asarray(r32[k][0]) - np.asarray(r64[k][0])).max()) for k in tc.OUTPUTS] + \
              [float(np.abs(r32[k] - r64[k]).max()) for k in tc.CHAINED]
        assert np.isfinite(err).all() and err == pytest.approx(GOLD["e_ref"][i].tolist(), rel=1e-6)
        for j, k in enumerate(tc.CHAINED):
            assert GOLD["e_ref"][i, len(tc.OUTPUTS) + j] >= tc.HALF_ULP * np.abs(r64[k]).max()


def test_the_hard_case_breaks_the_fp32_restatement():
    case = tc.HARD_CASE
    W, b = tc.layer(case[0])
    prompt, cand = tc.inputs(case, 0, scale=1.0)
    sel = tc.hard_selection()
    r32 = tc.run_torch(W, b, prompt, cand, tc.rewards(case, 0)[:1], case[4], torch.float32, sels=sel[None])
    assert not np.isfinite(r32["log_prob"][0]).all() and not np.isfinite(r32["grad_W"][0]).all()
    r64 = tc.ref64(case, 0, sel[None], stable=True, scale=1.0)
    assert all(np.isfinite(np.asarray(r64[k][0])).all() for k in tc.OUTPUTS)


# ------------------------------------------------------------------------------------------- train_batch, host logic
EXAMPLES = [{"captions": f"caption {i}", "label": ["cat", "mat"], "bbox": [[0.5, 0.4, 0.4, 0.3], [0.5, 0.8, 0.9, 0.25]]} for i in range(6)]
BATCH = [{"captions": f"train {i}", "label": ["dog"], "bbox": [[0.5, 0.5, 0.2, 0.4]], "image": f"img{i}"} for i in range(4)]
ANSWER = "dog: [0.10, 0.20, 0.30, 0.40]"


class Recorder:
    """stands for a PolicyTrainer: fixed probabilities, records the step's arguments"""

    def __init__(self, probs):
        self.probs, self.calls = probs, []
        self.policy = self

    def probabilities(self, emb, feats, temperature):
        self.seen = (tuple(emb.shape), tuple(feats.shape), temperature)
        return self.probs

    def step(self, emb, feats, sel, reward, temperature):
        self.calls.append((emb.clone(), np.asarray(sel).copy(), reward.clone(), temperature))
        return {"loss": torch.tensor(-2.5, dtype=torch.float64)}


def test_train_batch_draws_drops_and_orders_as_the_reference_does():
    probs = torch.softmax(torch.randn(4, 6, generator=torch.Generator().manual_seed(3)), 1)
    pool = CandidatePool(EXAMPLES, torch.zeros(6, 768))
    emb = torch.arange(4.0)[:, None].expand(4, 768).contiguous()
    seen = []

    def llm(text):
        seen.append(text)
        return "no layout, sorry: [1, 2, 3, 4]" if "input: train 1" in text else ANSWER

    made = {}

    def generate(captions, categories, bboxes):
        made["generate"] = (captions, categories, bboxes)
        return [f"pred{i}" for i in range(len(captions))]

    def reward(captions, images_pred, images_gt, layout_pred, layout_gt):
        made["reward"] = (captions, images_pred, images_gt, layout_pred, layout_gt)
        return torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)

    rec = Recorder(probs)
    np.random.seed(11)
    out = train_rl.train_batch(rec, pool, BATCH, emb, llm, generate, reward, shot_number=2, temperature=2.0)
    after = np.random.random()
    # the same draws from numpy's stream as sample_examples takes, row by row
    np.random.seed(11)
    want = [sample_examples(probs[i], 2) for i in range(4)]
    assert np.random.random() == after
    assert out["kept"] == [0, 2, 3] and out["cids"] == want[3].tolist() and out["reward"] == -0.5 and out["loss"] == -2.5
    assert rec.seen == ((4, 768), (6, 768), 2.0)
    # the prompt holds the drawn examples in the reversed order sample_examples returns (the first draw last) ...
    assert seen == [prompting.build_prompt([EXAMPLES[c] for c in want[i]], BATCH[i]) for i in range(4)]
    # ... and the step gets the kept rows with the draw order, un-reversed
    (e, sel, r, T), = rec.calls
    assert e[:, 0].tolist() == [0.0, 2.0, 3.0] and T == 2.0 and r.tolist() == [1.0, -2.0, 0.5]
    assert sel.tolist() == [want[i][::-1].tolist() for i in (0, 2, 3)]
    assert made["generate"] == (["train 0", "train 2", "train 3"], [["dog"]] * 3, [[[0.1, 0.2, 0.3, 0.4]]] * 3)
    caps, pred, gt, lp, lg = made["reward"]
    assert pred == ["pred0", "pred1", "pred2"] and gt == ["img0", "img2", "img3"]
    assert lp == [([[0.1, 0.2, 0.3, 0.4]], ["dog"])] * 3 and lg == [([[0.5, 0.5, 0.2, 0.4]], ["dog"])] * 3
    # every row dropped: no generation, no reward, no step
    rec2 = Recorder(probs)
    out = train_rl.train_batch(rec2, pool, BATCH, emb, lambda t: "nothing", lambda *a: 1 / 0, lambda *a: 1 / 0, rng=np.random.RandomState(0))
    assert out["kept"] == [] and out["reward"] == 0.0 and out["loss"] == 0.0 and rec2.calls == []
    with pytest.raises(ValueError, match="reward returned"):
        train_rl.train_batch(Recorder(probs), pool, BATCH, emb, lambda t: ANSWER, generate, reward, rng=np.random.RandomState(0))
    with pytest.raises(ValueError, match="records but emb_batch"):
        train_rl.train_batch(rec, pool, BATCH, emb[:3], llm, generate, reward)


def test_reward_adaptor_converts_the_ground_truth_boxes():
    class Model:
        def forward_layouts(self, ids, pred, gt, layout_pred, layout_gt, tokenize, attention_mask=None):
            self.got = (ids, attention_mask, layout_pred, layout_gt)
            return {"reward": torch.tensor([1.5], dtype=torch.float32)}
    m = Model()
    r = train_rl.reward_with(m, lambda texts: (len(texts), "mask"))(["a"], ["p"], ["g"], [([[0.1, 0.2, 0.3, 0.4]], ["dog"])], [([[0.5, 0.5, 0.2, 0.4]], ["dog"])])
    assert r.dtype == torch.float64 and r.tolist() == [1.5]
    assert m.got == (1, "mask", [([[0.1, 0.2, 0.3, 0.4]], ["dog"])], [(prompting.center2lefttop([[0.5, 0.5, 0.2, 0.4]]), ["dog"])])
