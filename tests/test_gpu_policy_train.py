"""Policy training on the GPU: gl_policy_grad and gl_policy_adam_step through PolicyTrainer against the fp64 run of the torch restatement
(tests/policy_train_cases.py) with the bound BOUND_FACTOR * e_ref of tests/golden/policy_train_ref.npz, the rules for skipped and repeated
selections, the hard range where the fp32 restatement gives -inf, determinism, resuming across the two implementations, and the loop of
train_rl.py executed on the synthetic tiny checkpoint.

Figures of an MI355X run (tools/policy_train_probe.py, profiles/policy_train_parity.txt): see that file; every ratio is printed below
before it is asserted."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import policy_cases as pc
import policy_train_cases as tc
from layoutllm_t2i_amd import train_rl
from layoutllm_t2i_amd.policy import CandidatePool, PolicyNetwork, sample_examples
from layoutllm_t2i_amd.policy_train import PolicyTrainer

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "policy_train_ref.npz"))
NAMES = GOLD["names"].tolist()
GOT = {"loss": "loss", "log_prob": "log_prob", "grad_W": "grad_weight", "grad_b": "grad_bias"}
RESUME_CASE = "d768_e128_n32_p8_k2_t0.5"


def trainer_for(config, lr=tc.LR, **kw):
    D, E = tc.CONFIGS[config]
    W, b = tc.layer(config)
    net = PolicyNetwork(D, E, device=DEV).load_state_dict({"weight": torch.from_numpy(W), "bias": torch.from_numpy(b)})
    return PolicyTrainer(net, lr=lr, **kw)


def recorded(name):
    i = NAMES.index(name)
    case, seed = tc.CASES[i], int(GOLD["seeds"][i])
    prompt, cand = tc.inputs(case, seed)
    return i, case, seed, torch.from_numpy(prompt).to(DEV), torch.from_numpy(cand).to(DEV), GOLD[name + ".sel"], GOLD[name + ".reward"]


def err(got, want) -> float:
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - np.asarray(want, np.float64)).max())


def state_of(tr):
    return {"W": tr.policy.weight, "bias": tr.policy.bias, "exp_avg_W": tr.exp_avg[0], "exp_avg_b": tr.exp_avg[1],
            "exp_avg_sq_W": tr.exp_avg_sq[0], "exp_avg_sq_b": tr.exp_avg_sq[1]}


# ------------------------------------------------------------------------------------------- parity
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_loss_and_gradient_are_within_the_references_own_error(name):
    i, case, seed, prompt, cand, sel, reward = recorded(name)
    r64 = tc.ref64(case, seed, sel)
    out = trainer_for(case[0]).loss_and_grad(prompt, cand, sel[0], reward[0], case[4])
    assert out["loss"].dtype == out["log_prob"].dtype == torch.float64 and out["loss"].dim() == 0 and out["grad_weight"].dtype == torch.float32
    fails = []
    for j, key in enumerate(tc.OUTPUTS):
        e, e_ref = err(out[GOT[key]], r64[key][0]), float(GOLD["e_ref"][i, j])
        print(f"{name} {key}: error {e:.3e}, e_ref {e_ref:.3e}, ratio {e / e_ref:.3f}")
        if not e <= pc.BOUND_FACTOR * e_ref:
            fails.append((key, e, e_ref))
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_chained_adam_steps_are_within_the_references_own_error(name):
    i, case, seed, prompt, cand, sel, reward = recorded(name)
    r64 = tc.ref64(case, seed, sel)
    tr = trainer_for(case[0])
    for s in range(tc.STEPS):
        tr.step(prompt, cand, sel[s], reward[s], case[4])
    assert tr.steps == tc.STEPS
    fails = []
    for j, (key, t) in enumerate(state_of(tr).items()):
        e, e_ref = err(t, r64[key]), float(GOLD["e_ref"][i, len(tc.OUTPUTS) + j])
        print(f"{name} {key} after {tc.STEPS} steps: error {e:.3e}, e_ref {e_ref:.3e}, ratio {e / e_ref:.3f}")
        if not e <= pc.BOUND_FACTOR * e_ref:
            fails.append((key, e, e_ref))
    assert not fails, fails


# ------------------------------------------------------------------------------------------- skipped and repeated entries, hard range
def derived_bound(out, r64):
    """no e_ref: |got - fp64| <= 2^-23 max|fp64| per output tensor (one fp32 rounding, and as much again for the double summation)"""
    for key in tc.OUTPUTS:
        want = np.asarray(r64[key][0], np.float64)
        got = out[GOT[key]]
        assert bool(torch.isfinite(got).all()), key
        e, bound = err(got, want), 2.0 ** -23 * float(np.abs(want).max())
        print(f"{key}: error {e:.3e}, bound {bound:.3e}")
        assert e <= bound, (key, e, bound)


@pytest.mark.gpu
def test_invalid_entries_are_skipped_and_repeated_ones_count_twice():
    case = ("d768_e128", 32, 8, 8, 1.0)
    N, P, k = case[1:4]
    prompt, cand = (torch.from_numpy(a).to(DEV) for a in tc.inputs(case, 0))
    reward = tc.rewards(case, 0)[0]
    reward[1] = -0.75                                             # (the zero of the drawn rewards would hide row 1)
    sel = np.stack([(np.arange(k) * 5 + 3 * p) % N for p in range(P)]).astype(np.int64)
    sel[0, [1, 6]] = -1, N                                        # two invalid entries
    sel[1, :] = [-1, N, -7, N + 100, 2 ** 31 - 1, -2 ** 31, N, -1]     # nothing valid
    sel[2, 3:] = sel[2, 0]                                        # one index six times
    sel[3, 7] = sel[3, 0]                                         # one index twice
    sel[4, :7] = -1                                               # a single valid entry, last
    W, b = tc.layer(case[0])
    r64 = tc.run_torch(W, b, prompt.cpu().numpy(), cand.cpu().numpy(), reward[None], case[4], torch.float64, sels=sel[None], stable=True)
    tr = trainer_for(case[0])
    out = tr.loss_and_grad(prompt, cand, sel, reward, case[4])
    derived_bound(out, r64)
    assert float(out["log_prob"][1]) == 0.0
    # the restriction itself: a row with invalid entries is the row of its valid entries, bit for bit (the same sum in the same order)
    short = tr.loss_and_grad(prompt[[0, 4]], cand, np.array([[v for v in sel[0] if 0 <= v < N] + [-1] * 2, [sel[4, 7]] + [N] * 7])[:, :6], reward[[0, 4]], case[4])
    assert torch.equal(short["log_prob"], out["log_prob"][[0, 4]])
    # twice the index is twice its log-probability
    one = tr.loss_and_grad(prompt[3:4], cand, sel[3:4, :1], reward[3:4], case[4])["log_prob"][0]
    rest = tr.loss_and_grad(prompt[3:4], cand, sel[3:4, 1:7], reward[3:4], case[4])["log_prob"][0]
    assert float(out["log_prob"][3]) == pytest.approx(float(2 * one + rest), rel=1e-14)
    # a batch of invalid rows only: zero loss, zero gradient
    none = tr.loss_and_grad(prompt, cand, np.full((P, 2), -1), reward, case[4])
    assert float(none["loss"]) == 0.0 and not none["log_prob"].any() and not none["grad_weight"].any() and not none["grad_bias"].any()


@pytest.mark.gpu
def test_hard_range_stays_finite_where_the_fp32_restatement_does_not():
    case = tc.HARD_CASE
    W, b = tc.layer(case[0])
    prompt, cand = tc.inputs(case, 0, scale=1.0)
    sel = tc.hard_selection()
    reward = tc.rewards(case, 0)
    r32 = tc.run_torch(W, b, prompt, cand, reward[:1], case[4], torch.float32, sels=sel[None])
    assert not np.isfinite(r32["log_prob"][0]).all() and not np.isfinite(r32["grad_W"][0]).all()
    r64 = tc.ref64(case, 0, sel[None], stable=True, scale=1.0)
    out = trainer_for(case[0]).loss_and_grad(torch.from_numpy(prompt), torch.from_numpy(cand), sel, reward[0], case[4])
    derived_bound(out, r64)


@pytest.mark.gpu
def test_the_largest_sizes_the_entry_accepts():
    """P = 64, N = 4096, D = E = 1024, k = 32: every limit of gl_policy_grad at once (68 MB of scratch), one update"""
    P, N, D, E, k, T = 64, 4096, 1024, 1024, 32, 2.0
    W = tc.recipe.normal("policy_train.max.W", (E, D), 0) / np.float32(np.sqrt(D))
    b = np.float32(0.1) * tc.recipe.normal("policy_train.max.b", (E,), 0)
    prompt = np.float32(0.3) * tc.recipe.normal("policy_train.max.prompt", (P, D), 0)
    cand = np.float32(0.3) * tc.recipe.normal("policy_train.max.cand", (N, D), 0)
    reward = tc.recipe.normal("policy_train.max.reward", (P,), 0).astype(np.float64)
    sel = np.stack([(np.arange(k) * 127 + 61 * p) % N for p in range(P)])
    sel[:, -1] = N - 1 - np.arange(P)                               # the last rows of the pool
    r64 = tc.run_torch(W, b, prompt, cand, reward[None], T, torch.float64, sels=sel[None], stable=True)
    net = PolicyNetwork(D, E, device=DEV).load_state_dict({"weight": torch.from_numpy(W), "bias": torch.from_numpy(b)})
    tr = PolicyTrainer(net, lr=tc.LR)
    out = tr.step(torch.from_numpy(prompt), torch.from_numpy(cand), sel, reward, T)
    derived_bound(out, r64)
    e, bound = err(net.weight, r64["W"]), 2.0 ** -23 * float(np.abs(r64["W"]).max())
    print(f"W after the step: error {e:.3e}, bound {bound:.3e}")
    assert e <= bound


# ------------------------------------------------------------------------------------------- determinism and independence
@pytest.mark.gpu
def test_two_calls_are_bit_equal_and_prompts_are_independent():
    name = "d768_e128_n65_p64_k32_t0.5"
    i, case, seed, prompt, cand, sel, reward = recorded(name)
    tr = trainer_for(case[0])
    w0, b0 = tr.policy.weight.clone(), tr.policy.bias.clone()
    a = tr.loss_and_grad(prompt, cand, sel[0], reward[0], case[4])
    b = tr.loss_and_grad(prompt, cand, torch.from_numpy(sel[0]).to(DEV), torch.from_numpy(reward[0]).float().to(DEV), case[4])
    for key in a:
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(tr.policy.weight, w0) and torch.equal(tr.policy.bias, b0) and tr.steps == 0       # loss_and_grad leaves the layer alone
    perm = np.random.RandomState(5).permutation(case[2])
    c = tr.loss_and_grad(prompt[perm], cand, sel[0][perm], reward[0][perm], case[4])
    assert torch.equal(c["log_prob"], a["log_prob"][perm])
    r64 = tc.ref64(case, seed, sel)
    for j, key in ((2, "grad_W"), (3, "grad_b")):
        e, e_ref = err(c[GOT[key]], r64[key][0]), float(GOLD["e_ref"][i, j])
        print(f"permuted prompts, {key}: error {e:.3e}, e_ref {e_ref:.3e}, ratio {e / e_ref:.3f}")
        assert e <= pc.BOUND_FACTOR * e_ref
    # after a step the policy scores with the new layer: the same scores as a fresh network loaded with the saved weights
    before = tr.policy.scores(prompt, cand)
    tr.step(prompt, cand, sel[0], reward[0], case[4])
    assert not torch.equal(tr.policy.weight, w0) and tr.steps == 1
    fresh = PolicyNetwork(*tc.CONFIGS[case[0]], device=DEV).load_state_dict(tr.weights())
    after = tr.policy.scores(prompt, cand)
    assert torch.equal(after, fresh.scores(prompt, cand)) and not torch.equal(after, before)


# ------------------------------------------------------------------------------------------- resume across implementations
@pytest.mark.gpu
def test_a_run_resumes_in_torch_and_torchs_run_resumes_here():
    i, case, seed, prompt, cand, sel, reward = recorded(RESUME_CASE)
    D, E = tc.CONFIGS[case[0]]
    bound = {k: pc.BOUND_FACTOR * float(GOLD["e_ref"][i, len(tc.OUTPUTS) + j]) for j, k in enumerate(tc.CHAINED)}
    W, b = tc.layer(case[0])
    x, y = prompt.cpu().numpy(), cand.cpu().numpy()
    # three steps here, then two more on both sides
    tr = trainer_for(case[0])
    for s in range(3):
        tr.step(prompt, cand, sel[s], reward[s], case[4])
    lin = torch.nn.Linear(D, E)
    lin.load_state_dict(tr.weights())
    opt = torch.optim.Adam(lin.parameters(), lr=123.0)
    state = tr.state_dict()
    opt.load_state_dict(state["optimizer"])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)
    sched.load_state_dict(state["lr_scheduler"])
    assert opt.param_groups[0]["lr"] == tc.LR and float(opt.state[lin.weight]["step"]) == 3 and sched.step_size == 20
    r32 = tc.run_torch(W, b, x, y, reward[3:], case[4], torch.float32, sels=sel[3:], linear=lin, optimizer=opt)
    for s in range(3, tc.STEPS):
        tr.step(prompt, cand, sel[s], reward[s], case[4])
    for key, t in state_of(tr).items():
        e = err(t, r32[key])
        print(f"here -> torch, {key}: difference {e:.3e}, bound {bound[key]:.3e}")
        assert e <= bound[key], key
    assert float(opt.state[lin.weight]["step"]) == tr.steps == 5
    # three steps in torch, then two more on both sides
    t32 = tc.run_torch(W, b, x, y, reward[:3], case[4], torch.float32, sels=sel[:3])
    sched = torch.optim.lr_scheduler.StepLR(t32["optimizer"], step_size=20, gamma=0.5)
    tr2 = trainer_for(case[0], lr=55.0)
    tr2.policy.load_state_dict(t32["linear"].state_dict())
    tr2.load_state_dict({"optimizer": t32["optimizer"].state_dict(), "lr_scheduler": sched.state_dict()})
    assert (tr2.steps, tr2.lr, tr2.base_lr) == (3, tc.LR, tc.LR)
    t32 = tc.run_torch(W, b, x, y, reward[3:], case[4], torch.float32, sels=sel[3:], linear=t32["linear"], optimizer=t32["optimizer"])
    for s in range(3, tc.STEPS):
        tr2.step(prompt, cand, sel[s], reward[s], case[4])
    for key, t in state_of(tr2).items():
        e = err(t, t32[key])
        print(f"torch -> here, {key}: difference {e:.3e}, bound {bound[key]:.3e}")
        assert e <= bound[key], key


# ------------------------------------------------------------------------------------------- the loop
POOL = [{"captions": c, "label": l, "bbox": b} for c, l, b in (
    ("a cat on a mat", ["cat", "mat"], [[0.5, 0.4, 0.4, 0.3], [0.5, 0.8, 0.9, 0.25]]),
    ("two dogs under a tree", ["dog", "dog", "tree"], [[0.25, 0.6, 0.25, 0.25], [0.6, 0.62, 0.3, 0.3], [0.5, 0.3, 0.8, 0.6]]),
    ("a quiet empty street", ["street"], [[0.5, 0.75, 1.0, 0.5]]),
    ("a red car at night", ["car"], [[0.4, 0.6, 0.5, 0.3]]),
    ("a big dog sitting on a mat", ["dog", "mat"], [[0.5, 0.5, 0.3, 0.4], [0.5, 0.85, 0.8, 0.2]]),
    ("a tree", ["tree"], [[0.5, 0.5, 0.6, 0.9]]),
)]
TRAIN = [{"captions": c, "label": ["cat"], "bbox": [[0.5, 0.5, 0.4, 0.4]], "image": None} for c in
         ("a cat by a window", "nothing to draw here", "a dog and a cat", "a car under a tree")]
ANSWERS = {"a cat by a window": "cat: [0.10, 0.10, 0.40, 0.45]\nwindow: [0.55, 0.20, 0.35, 0.50]", "nothing to draw here": "I cannot: [1, 2, 3, 4]",
           "a dog and a cat": "dog: [0.05, 0.30, 0.40, 0.50]\ncat: [0.50, 0.35, 0.45, 0.40]", "a car under a tree": "car: [0.20, 0.55, 0.50, 0.30]"}
LOOP_T = 2.0


def llm(text):
    query = text.rsplit("input: ", 1)[1]
    return next(a for c, a in ANSWERS.items() if query.startswith(c))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import stubs
    from layoutllm_t2i_amd import interface as itf
    from layoutllm_t2i_amd.arch import TINY, VAE_TINY
    p = str(tmp_path_factory.mktemp("ckpt") / "tiny_gligen.pth")
    stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)
    stubs.install_fake_sng_parser()
    am = itf.load_all_models(p, DEV)
    clip, proc = stubs.toy_clip().to(DEV), stubs.ToyProcessor()
    rewards = []

    def generate(captions, categories, bboxes):
        n = len(captions)
        args = dict(batch_size=n, no_plms=False, guidance_scale=7.5, steps=2)
        meta = dict(prompts=captions, phrases=categories, locations=bboxes, alpha_type=[0.3, 0.0, 0.7])
        noise = torch.randn(n, 4, 16, 16, generator=torch.Generator().manual_seed(n))
        return itf.run_batch_images(am, args, meta, noise.to(DEV), clip, proc, device=DEV)

    def reward(captions, images_pred, images_gt, layout_pred, layout_gt):
        assert len(images_pred) == len(captions) == len(layout_gt) and images_pred[0].size == (32, 32)
        r = torch.tensor([np.asarray(im, np.float64).mean() / 255.0 - 0.5 + 0.25 * len(lp[0]) for im, lp in zip(images_pred, layout_pred)], dtype=torch.float64)
        rewards.append(r)
        return r.to(DEV)

    feats = np.float32(0.3) * tc.recipe.normal("policy_train.loop.pool", (len(POOL), 768), 0)
    emb = torch.from_numpy(np.float32(0.3) * tc.recipe.normal("policy_train.loop.train", (len(TRAIN), 768), 0)).to(DEV)
    return CandidatePool(POOL, torch.from_numpy(feats).to(DEV)), emb, generate, reward, rewards


@pytest.mark.gpu
def test_train_batch_is_one_trainer_step_on_the_kept_rows(world):
    pool, emb, generate, reward, rewards = world
    tr = trainer_for("d768_e128", lr=1e-3)
    probs = tr.policy.probabilities(emb, pool.features, LOOP_T).cpu()
    del rewards[:]
    out = train_rl.train_batch(tr, pool, TRAIN, emb, llm, generate, reward, shot_number=2, temperature=LOOP_T, rng=np.random.RandomState(21))
    assert out["kept"] == [0, 2, 3] and tr.steps == 1 and len(rewards) == 1                     # the row without a box is dropped
    assert out["reward"] == float(rewards[0].sum()) and np.isfinite(out["loss"]) and out["loss"] != 0.0
    # the same update from trainer.step directly, bit for bit
    rng = np.random.RandomState(21)
    drawn = [sample_examples(probs[i], 2, rng) for i in range(4)]
    assert out["cids"] == drawn[3].tolist()
    tr2 = trainer_for("d768_e128", lr=1e-3)
    res = tr2.step(emb[[0, 2, 3]], pool.features, np.stack([drawn[i][::-1] for i in (0, 2, 3)]), rewards[0], LOOP_T)
    assert float(res["loss"]) == out["loss"]
    for (key, a), b in zip(state_of(tr).items(), state_of(tr2).values()):
        assert torch.equal(a, b), key


@pytest.mark.gpu
def test_policy_gradient_train_writes_the_references_files_and_resumes(world, tmp_path):
    pool, emb, generate, reward, rewards = world
    first, second = str(tmp_path / "run1"), str(tmp_path / "run2")
    kw = dict(shot_number=2, temperature=LOOP_T)
    tr = trainer_for("d768_e128", lr=1e-4, lr_step_size=2, lr_gamma=0.5)
    hist = train_rl.policy_gradient_train(tr, pool, TRAIN, emb, llm, generate, reward, first, epochs=2, batch_size=2,
                                          rng=np.random.RandomState(3), **kw)
    assert sorted(os.listdir(first)) == sorted(["ckpt_0.pt", "ckpt_1.pt", "state_0.pt", "state_1.pt", "ckpt_best_reward.pt", "ckpt_best_loss.pt",
                                                 "ckpt_final.pt", "history.json"])
    on_disk = json.load(open(os.path.join(first, "history.json")))
    assert set(on_disk) == {"reward_history", "loss_history", "total_reward_history", "total_loss_history"}
    assert len(on_disk["reward_history"]) == len(on_disk["loss_history"]) == 4 and len(on_disk["total_reward_history"]) == 2
    assert on_disk["total_loss_history"][1] == on_disk["loss_history"][2] + on_disk["loss_history"][3]
    assert (hist["start_epoch"], hist["last_epoch"], tr.steps, tr.epochs, tr.lr) == (0, 1, 4, 2, 0.5e-4)
    final = torch.load(os.path.join(first, "ckpt_final.pt"), weights_only=True)
    assert set(final) == {"weight", "bias"} and torch.equal(final["weight"], tr.policy.weight.cpu())
    state = torch.load(os.path.join(first, "state_1.pt"), weights_only=True)
    assert set(state) == {"optimizer", "lr_scheduler"} and float(state["optimizer"]["state"][0]["step"]) == 4
    assert state["optimizer"]["param_groups"][0]["lr"] == 1e-4 and state["lr_scheduler"]["last_epoch"] == 1        # written before the epoch's scheduler step
    best = on_disk["total_reward_history"].index(max(on_disk["total_reward_history"]))
    assert torch.equal(torch.load(os.path.join(first, "ckpt_best_reward.pt"), weights_only=True)["weight"],
                       torch.load(os.path.join(first, f"ckpt_{best}.pt"), weights_only=True)["weight"])
    # a fresh trainer resumes: epoch 2, step 5 and 6, the halved learning rate
    tr2 = trainer_for("d768_e128", lr=7.0)
    hist2 = train_rl.policy_gradient_train(tr2, pool, TRAIN, emb, llm, generate, reward, second, epochs=1, batch_size=2, resume=first,
                                           rng=np.random.RandomState(4), **kw)
    assert (hist2["start_epoch"], hist2["last_epoch"], tr2.steps, tr2.epochs, tr2.lr, tr2.base_lr) == (2, 2, 6, 3, 0.5e-4, 1e-4)
    assert {"ckpt_2.pt", "state_2.pt", "ckpt_final.pt", "history.json"} <= set(os.listdir(second))
    state2 = torch.load(os.path.join(second, "state_2.pt"), weights_only=True)
    assert float(state2["optimizer"]["state"][1]["step"]) == 6 and state2["optimizer"]["param_groups"][0]["lr"] == 0.5e-4
    assert not torch.equal(torch.load(os.path.join(second, "ckpt_2.pt"), weights_only=True)["weight"], final["weight"])
    # the reference's "use new learning rate": the schedule starts again from it
    tr3 = trainer_for("d768_e128")
    train_rl.resume_from(tr3, first)
    tr3.set_lr(3e-4)
    assert (tr3.steps, tr3.lr, tr3.epochs) == (4, 3e-4, 0) and torch.equal(tr3.policy.weight.cpu(), final["weight"])
