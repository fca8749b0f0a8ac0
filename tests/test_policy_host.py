"""Prompt-to-image entry, host side (no GPU): the C ABI of gl_policy_select and its refusals, PolicyNetwork's checkpoint check, the
rollout's sampling against the test's own restatement of train_rl.py:38-48, and the prompt text work against the recorded results
of the reference's base_prompt.build_prompt / utils.extract_prediction / utils.center2lefttop (tests/golden/prompting_ref.json,
tools/make_policy_goldens.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import policy_cases as pc
from layoutllm_t2i_amd import _lib, interface, policy, prompting
from layoutllm_t2i_amd.policy import CandidatePool, PolicyNetwork, sample_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = json.load(open(os.path.join(ROOT, "tests", "golden", "prompting_ref.json")))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "policy_ref.npz"))


def _built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)
    return _lib.lib()


# ------------------------------------------------------------------------------------------- C ABI
def test_policy_entries_are_exported_under_abi_15():
    l = _built()
    assert l.gl_sizeof_policy_args() == ctypes.sizeof(_lib.PolicyArgs) == 104
    assert l.gl_abi_version() == _lib.ABI_VERSION == 15
    hdr = open(os.path.join(ROOT, "include", "gligen_hip.h")).read()
    for fn in ("gl_policy_select", "gl_sizeof_policy_args", "gl_policy_scratch_bytes"):
        assert fn in _lib.PROTOTYPES and hasattr(l, fn) and f" {fn}(" in hdr, fn
    assert "#define GL_POLICY_MAX_SHOTS 32" in hdr and "#define GL_POLICY_MAX_PROMPTS 64" in hdr and "#define GL_POLICY_MAX_DIM 1024" in hdr
    assert (policy.MAX_SHOTS, policy.MAX_PROMPTS, policy.MAX_DIM) == (32, 64, 1024)
    assert "policy.hip" in __import__("layoutllm_t2i_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


def test_policy_scratch_size():
    l = _built()
    a256 = lambda b: (b + 255) // 256 * 256
    for P, N, D, E, k in ((1, 1, 768, 128, 0), (3, 65, 768, 128, 2), (64, 4099, 512, 128, 32), (16, 82783, 768, 128, 2)):
        blocks = (N + 63) // 64
        fold, local = a256(P * E * 8) + a256(P * D * 4) + a256(P * 4), a256(P * blocks * k * 8)
        assert l.gl_policy_scratch_bytes(P, N, D, E, k, 0, 0) == fold + local
        assert l.gl_policy_scratch_bytes(P, N, D, D, k, 1, 0) == local
        # probabilities: the unrounded fold and the scores in double
        assert l.gl_policy_scratch_bytes(P, N, D, E, k, 0, 1) == fold + a256(P * D * 8) + a256(P * 8) + a256(P * N * 8) + local
        assert l.gl_policy_scratch_bytes(P, N, D, D, k, 1, 1) == a256(P * N * 8) + local
    for bad in ((0, 1, 4, 4, 0), (1, 0, 4, 4, 0), (1, 1, 0, 4, 0), (1, 1, 4, 0, 0), (1, 1, 4, 4, -1)):
        assert l.gl_policy_scratch_bytes(*bad, 0, 0) == -1


def test_policy_select_refuses_bad_arguments_before_any_launch():
    """every refusal is decided on the host from the struct: nothing is launched, so this runs without a GPU (the pointers that
    stand for device memory are never read)"""
    l = _built()
    dev = (ctypes.c_double * 8)()                       # 16-byte aligned below; refusals never dereference it
    p = (ctypes.addressof(dev) + 15) // 16 * 16

    def args(**kw):
        a = _lib.PolicyArgs()
        a.prompt = a.cand = a.W = a.bias = a.scores = a.topk = a.probs = a.scratch = p
        a.P, a.N, a.D, a.E, a.k, a.temperature, a.scratch_bytes = 3, 65, 768, 128, 2, 1.0, 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(what, **kw):
        assert l.gl_policy_select(ctypes.byref(args(**kw)), None) == -1, kw
        msg = _lib.last_error(None)
        assert msg.startswith("gl_policy_select:") and what in msg, (kw, msg)

    assert l.gl_policy_select(None, None) == -1 and "null args" in _lib.last_error(None)
    for field in ("prompt", "cand", "bias", "scores", "topk", "scratch"):
        refused("null", **{field: None})
    refused("P = 0", P=0)
    refused("P = 65", P=65)
    refused("N = 0", N=0)
    refused("N = -3", N=-3)
    for D in (0, 2, 766, 1028, -4):
        refused(f"D = {D}", D=D)
    refused("E = 0", E=0)
    refused("E = 1025", E=1025)
    refused("E = 128 with W == NULL", W=None, bias=None)        # the identity needs E == D
    refused("k = -1", k=-1)
    refused("k = 33", k=33)
    for t in (0.0, -1.0, float("nan")):
        refused("temperature", temperature=t)
    need = l.gl_policy_scratch_bytes(3, 65, 768, 128, 2, 0, 1)
    refused(f"needs {need}", scratch_bytes=need - 1)
    refused("16-byte aligned", cand=p + 4)
    # what is allowed: no probs (temperature unread), no bias with the identity, the largest sizes -- refused only further on, here for the scratch
    refused("scratch of 0 bytes", k=1, probs=None, temperature=0.0, W=None, bias=None, E=1024, scratch_bytes=0, P=64, N=(1 << 31) - 1, D=1024)
    # a layout-reward refusal and a policy refusal share the calling thread's message slot
    assert l.gl_layout_reward(None, None) == -1 and _lib.last_error(None).startswith("gl_layout_reward:")


# ------------------------------------------------------------------------------------------- PolicyNetwork / CandidatePool / sampling
def test_policy_network_checks_the_checkpoint():
    net = PolicyNetwork(in_dim=768, embedding_size=128, device="cpu")
    sd = {"weight": torch.zeros(128, 768), "bias": torch.zeros(128)}
    assert net.load_state_dict(sd) is net and net.weight.shape == (128, 768) and net.weight.dtype == torch.float32
    for bad in ({"weight": torch.zeros(768, 128), "bias": torch.zeros(128)}, {"weight": torch.zeros(128, 768), "bias": torch.zeros(768)},
                {"weight": torch.zeros(128, 512), "bias": torch.zeros(128)}, {"weight": torch.zeros(128 * 768), "bias": torch.zeros(128)}):
        with pytest.raises(ValueError, match=r"expected \(128, 768\) / \(128,\)"):
            net.load_state_dict(bad)
    with pytest.raises(ValueError, match="without"):
        net.load_state_dict({"linear.weight": sd["weight"], "linear.bias": sd["bias"]})
    with pytest.raises(ValueError, match="no layer"):
        PolicyNetwork(add_linear=False, device="cpu").load_state_dict(sd)
    for kw in (dict(in_dim=770), dict(in_dim=1028), dict(in_dim=0), dict(embedding_size=0), dict(embedding_size=1025)):
        with pytest.raises(ValueError):
            PolicyNetwork(device="cpu", **kw)
    # shapes and ranges are checked before a device is needed; the scoring itself has no CPU form
    with pytest.raises(ValueError, match="emb_cand"):
        net.scores(torch.zeros(2, 768), torch.zeros(5, 512))
    with pytest.raises(ValueError, match="shot_number"):
        net.select(torch.zeros(2, 768), torch.zeros(5, 768), 33)
    with pytest.raises(ValueError, match="temperature"):
        net.probabilities(torch.zeros(2, 768), torch.zeros(5, 768), 0.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        net.scores(torch.zeros(2, 768), torch.zeros(5, 768))
    assert net.select(torch.zeros(2, 768), torch.zeros(5, 768), 0).shape == (2, 0)


def test_candidate_pool_checks_its_sizes():
    ex = [{"captions": "a", "label": [], "bbox": []}] * 3
    assert len(CandidatePool(ex, torch.zeros(3, 8))) == 3
    with pytest.raises(ValueError, match="3 examples but features"):
        CandidatePool(ex, torch.zeros(4, 8))
    with pytest.raises(ValueError, match="empty"):
        CandidatePool([], torch.zeros(0, 8))


def test_sample_examples_is_the_rollout_of_the_reference():
    """the test's restatement of train_rl.py:38-48: nan_to_num, renormalise, np.random.choice without replacement, reverse"""
    rows = [torch.softmax(torch.randn(32, generator=torch.Generator().manual_seed(s)) * 3, 0) for s in range(3)]
    rows[1][5] = float("nan")
    rows[2][[0, 31]] = float("nan")
    for seed, (row, k) in enumerate(zip(rows, (2, 4, 1))):
        np.random.seed(100 + seed)
        cand_prob = row.clone().detach().cpu().numpy()
        cand_prob = np.nan_to_num(cand_prob, nan=0.000001)
        cand_prob /= cand_prob.sum()
        want = np.random.choice(range(len(cand_prob)), k, p=cand_prob, replace=False)[::-1]
        after = np.random.random()
        np.random.seed(100 + seed)
        got = sample_examples(row, k)
        assert got.tolist() == want.tolist() and len(set(got.tolist())) == k
        assert np.random.random() == after                       # the same draws were taken from numpy's stream
        assert torch.isnan(row).sum() == (0, 1, 2)[seed]          # the caller's row is untouched
    rs = np.random.RandomState(7)
    assert sample_examples(rows[0], 3, rs).tolist() == np.random.RandomState(7).choice(range(32), 3, p=_p(rows[0]), replace=False)[::-1].tolist()


def _p(row):
    p = np.nan_to_num(row.numpy().copy(), nan=0.000001)
    return p / p.sum()


# ------------------------------------------------------------------------------------------- cases and goldens
def test_policy_golden_file_matches_the_regenerated_cases():
    names = GOLD["names"].tolist()
    assert names[:len(pc.CASES)] == [pc.case_name(c) for c in pc.CASES] and names[len(pc.CASES):] == list(pc.TIE_CASES)
    assert len(pc.CASES) == 72 and {c[1] for c in pc.CASES} == {1, 32, 63, 64, 65, 4099} and {c[2] for c in pc.CASES} == {1, 3, 8, 64}
    assert (GOLD["e_ref"] > 0).all() and (GOLD["gap"] > pc.GAP_FACTOR * GOLD["e_ref"]).all()
    assert (GOLD["e_ref"] < 1e-6 * GOLD["max_abs"]).all()          # the reference's fp32 evaluation: a few 1e-7 of the largest score
    for name in ("d768_e128_n65_p3", "d512_e128_n32_p64", "d768_identity_n63_p8", "d768_e128_n64_p64"):
        i = names.index(name)
        case = pc.CASES[i]
        prompt, cand = pc.inputs(case, int(GOLD["seeds"][i]))
        s = pc.scores64(case[0], prompt, cand)
        assert abs(s.sum() - GOLD["checksum"][i]) <= 1e-9 * abs(GOLD["checksum"][i]) + 1e-9 and np.abs(s).max() == pytest.approx(GOLD["max_abs"][i], rel=1e-12)
        order = pc.ranking(s)
        assert order[0, :pc.RANKS].tolist() == [v for v in GOLD["top0"][i].tolist() if v >= 0]
        v, c = pc.folded(case[0], prompt)
        assert np.abs(cand.astype(np.float64) @ v.T + c - s.T).max() <= 1e-9 * np.abs(s).max()      # the folded form is the same function
    case, prompt, cand = pc.tie_inputs("ties_n65_k2", 0)
    order = pc.ranking(pc.scores64(case[0], prompt, cand))[0]
    assert np.array_equal(cand[order[0]], cand[order[1]]) and order[0] < order[1] == 64           # the copy in the second block ranks second
    assert np.array_equal(cand[order[2]], cand[order[3]]) and order[2] < order[3]


# ------------------------------------------------------------------------------------------- prompt text
@pytest.mark.parametrize("name", sorted(REF["prompts"]))
def test_build_prompt_equals_the_recorded_reference_prompt(name):
    rec = REF["prompts"][name]
    got = prompting.build_prompt(rec["shot_cand"], {"captions": REF["caption"]}, instruction=REF["instruction"])
    assert got == rec["prompt"]
    assert got.count("\ninput: ") == len(rec["shot_cand"]) + 1 and got.count("output: \n") == len(rec["shot_cand"])


def test_prompt_cases_cover_rounding_and_a_negative_corner():
    assert sorted(len(v["shot_cand"]) for v in REF["prompts"].values()) == [0, 1, 1, 3]
    p = REF["prompts"]["dot_x5_and_negative_corner"]["prompt"]
    assert "dog: [0.12, 0.38, 0.25, 0.25]" in p and "dog: [-0.05, 0.36, 0.7, 0.51]" in p       # round-half-even on the binary values
    assert "traffic light: [0.75, 0.05, 0.11, 0.33]" in REF["prompts"]["three_shots"]["prompt"]


def test_default_instruction_is_this_projects_own_wording():
    d = prompting.DEFAULT_INSTRUCTION
    assert d["few_shot"] and d["zero_shot"] and d["few_shot"] != d["zero_shot"] and d["query_note"]
    for key in d:
        assert d[key] != REF["instruction"][key]
    zero = prompting.build_prompt([], {"captions": "a dog"})
    few = prompting.build_prompt(REF["prompts"]["one_shot"]["shot_cand"], {"captions": "a dog"})
    assert zero.startswith(d["zero_shot"]) and few.startswith(d["few_shot"]) and zero.endswith("input: a dog" + d["query_note"])
    assert "cat: [0.3, 0.25, 0.4, 0.3]" in few and "[x, y, w, h]" in zero
    # a plain string replaces the preamble of either form; unknown keys are refused
    assert prompting.build_prompt([], {"captions": "a dog"}, "DO IT").startswith("DO IT\n\ninput: a dog")
    with pytest.raises(ValueError, match="instruction keys"):
        prompting.build_prompt([], {"captions": "a dog"}, {"preamble": "x"})


@pytest.mark.parametrize("name", sorted(REF["answers"]))
def test_extract_prediction_equals_the_recorded_reference_result(name):
    rec = REF["answers"][name]
    cats, boxes = prompting.extract_prediction(rec["text"])
    assert cats == rec["categories"] and boxes == rec["bboxes"]


def test_extract_prediction_cases_hit_the_edges_of_the_pattern():
    a = REF["answers"]
    assert a["one_and_two_words"]["categories"] == ["cat", "traffic light"] and a["one_and_two_words"]["bboxes"][0] == [0.1, 0.2, 0.3, 0.4]
    assert a["three_words"]["categories"] == ["red car"]
    assert a["integer_skipped"]["categories"] == ["dog"] and a["negative_skipped"]["categories"] == ["dog"]
    assert a["extra_spaces"]["categories"] == ["potted   plant"] and a["two_on_one_line"]["categories"] == ["cat", "dog"]
    assert a["no_match"]["categories"] == [] == a["no_match"]["bboxes"] and a["empty"]["bboxes"] == []
    assert a["prose_around"]["categories"] == ["sofa", "lamp "]          # a space before the colon stays in the name
    assert a["trailing_comma_inside"]["categories"] == []


def test_box_helpers():
    assert prompting.center2lefttop(REF["center2lefttop"]["boxes"]) == REF["center2lefttop"]["result"]
    assert prompting.convert_xywh_to_ltrb is interface.convert_xywh_to_ltrb and prompting.convert_xcycwh_to_ltrb is interface.convert_xcycwh_to_ltrb
    assert prompting.convert_xywh_to_ltrb([0.1, 0.2, 0.3, 0.4]) == [0.1, 0.2, 0.1 + 0.3, 0.2 + 0.4]
    assert prompting.convert_xcycwh_to_ltrb([0.5, 0.5, 0.2, 0.4]) == [0.4, 0.3, 0.6, 0.7]
