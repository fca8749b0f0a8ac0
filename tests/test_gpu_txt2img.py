"""The prompt-to-image entry EXECUTED (txt2img.generate, the reference's txt2img.py:460-508) on the synthetic tiny checkpoint and the
stubs of test_boundary.py (16 x 16 latent, 4 PLMS steps): a toy CLIP text tower embeds the pool and the prompt, the policy kernel
selects, a stub ``llm`` answers with a canned layout, and the images must be the ones ``run_one_image`` makes from that layout."""
import dataclasses
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import policy_cases as pc
import stubs
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import recipe, txt2img
from layoutllm_t2i_amd.arch import TINY, VAE_TINY
from layoutllm_t2i_amd.policy import CandidatePool, PolicyNetwork
from layoutllm_t2i_amd.prompting import build_prompt

DEV = "cuda:0"
PROMPT = "cat sitting on mat and dog under a tree"
ANSWER = "output:\ncat: [0.10, 0.10, 0.40, 0.45]\nmat: [0.05, 0.60, 0.90, 0.35]\na big dog: [0.55, 0.20, 0.35, 0.50]\nbird: [1, 0.2, 0.3, 0.4]"
EXAMPLES = [{"captions": c, "label": l, "bbox": b} for c, l, b in (
    ("a cat on a mat", ["cat", "mat"], [[0.5, 0.4, 0.4, 0.3], [0.5, 0.8, 0.9, 0.25]]),
    ("two dogs under a tree", ["dog", "dog", "tree"], [[0.25, 0.6, 0.25, 0.25], [0.6, 0.62, 0.3, 0.3], [0.5, 0.3, 0.8, 0.6]]),
    ("a quiet empty street", ["street"], [[0.5, 0.75, 1.0, 0.5]]),
    ("a red car at night", ["car"], [[0.4, 0.6, 0.5, 0.3]]),
    ("a big dog sitting on a mat", ["dog", "mat"], [[0.5, 0.5, 0.3, 0.4], [0.5, 0.85, 0.8, 0.2]]),
    ("a tree", ["tree"], [[0.5, 0.5, 0.6, 0.9]]),
)]


def tokenize(texts):
    t = stubs.ToyProcessor()(text=list(texts))
    return t["input_ids"], t["attention_mask"]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from layoutllm_t2i_amd.clip import ClipTowers
    p = str(tmp_path_factory.mktemp("ckpt") / "tiny_gligen.pth")
    stubs.write_synthetic_checkpoint(p, TINY, VAE_TINY, max_relations=10)
    stubs.install_fake_sng_parser()
    am = itf.load_all_models(p, DEV)
    sd = stubs.toy_text_tower_state_dict(4)
    sd["text_projection.weight"] = torch.from_numpy(recipe.normal("txt2img.tproj", (768, 768), 4)) / np.sqrt(768.0)
    towers = ClipTowers(sd, text_heads=12, device=DEV)
    pool = CandidatePool.from_captions(EXAMPLES, towers, tokenize, batch=4)
    W, b = pc.layer("d768_e128")
    policy = PolicyNetwork(768, 128, device=DEV).load_state_dict({"weight": torch.from_numpy(W), "bias": torch.from_numpy(b)})
    return am, stubs.toy_clip().to(DEV), stubs.ToyProcessor(), towers, pool, policy


class StubLLM:
    def __init__(self, answer):
        self.answer, self.seen = answer, []

    def __call__(self, prompt_text):
        self.seen.append(prompt_text)
        return self.answer


def fp64_cids(towers, pool, k):
    """the reference's selection (txt2img.py:472-474, :429-431) in fp64 on the features the pool holds"""
    emb = towers.get_text_features(*tokenize([PROMPT])).clone()
    s = pc.scores64("d768_e128", emb.cpu().numpy(), pool.features.cpu().numpy())
    gaps = np.diff(np.sort(s[0])[::-1])
    assert np.abs(gaps).min() > 1e-3 * np.abs(s).max()                      # no near-tie among the six candidates
    return pc.ranking(s)[0, :k][::-1].tolist()


@pytest.mark.gpu
def test_generate_selects_prompts_parses_and_generates(setup, tmp_path):
    am, clip, proc, towers, pool, policy = setup
    llm = StubLLM(ANSWER)
    torch.manual_seed(7)
    noise = torch.randn(3, 4, 16, 16)
    am[0].first_conv_type = "GLIGEN"                                       # (sticky in the reference: the first scale-0 step switches it to SD)
    out = txt2img.generate(am, policy, pool, PROMPT, llm, tokenize, clip, proc, shot_number=2, num_per_prompt=3, batch_size=2, steps=4,
                           starting_noise=noise, folder=str(tmp_path / "out"), device=DEV)
    cids = fp64_cids(towers, pool, 2)
    assert out["cids"] == cids and len(set(cids)) == 2
    want_prompt = build_prompt([EXAMPLES[c] for c in cids], {"captions": PROMPT})
    assert llm.seen == [want_prompt] and out["prompt_text"] == want_prompt and out["llm_output"] == ANSWER
    assert want_prompt.index(EXAMPLES[cids[0]]["captions"]) < want_prompt.index(EXAMPLES[cids[1]]["captions"])    # the best example last
    assert out["categories"] == ["cat", "mat", "big dog"]                  # the name keeps two words; the integer item is skipped
    ltrb = [[0.10, 0.10, 0.10 + 0.40, 0.10 + 0.45], [0.05, 0.60, 0.05 + 0.90, 0.60 + 0.35], [0.55, 0.20, 0.55 + 0.35, 0.20 + 0.50]]
    assert out["bboxes_ltrb"] == ltrb
    assert len(out["images"]) == 3 and out["images"][0].size == (32, 32) and out["images"][0].mode == "RGB"
    # the same images as run_one_image, called directly with the parsed layout, the same noise rows and the same batches
    meta = dict(prompt=PROMPT, phrases=["cat", "mat", "big dog"], locations=ltrb, alpha_type=[0.3, 0.0, 0.7])
    direct = []
    am[0].first_conv_type = "GLIGEN"
    for lo, n in ((0, 2), (2, 1)):
        args = dict(batch_size=n, no_plms=False, guidance_scale=7.5, steps=4)
        direct += itf.run_one_image(am, args, meta, noise[lo:lo + n].to(DEV), clip, proc, device=DEV)
    for a, b in zip(out["images"], direct):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert not np.array_equal(np.asarray(out["images"][0]), np.asarray(out["images"][1]))
    saved = sorted(os.listdir(tmp_path / "out"))
    assert saved == [f"{PROMPT}_{i}.jpg" for i in range(3)]


@pytest.mark.gpu
def test_generate_is_center_converts_differently_and_zero_shot_runs(setup):
    am, clip, proc, towers, pool, policy = setup
    llm = StubLLM("cat: [0.5, 0.5, 0.4, 0.2]")
    noise = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(1))
    kw = dict(shot_number=0, num_per_prompt=1, steps=4, starting_noise=noise, device=DEV)
    xywh = txt2img.generate(am, policy, pool, PROMPT, llm, tokenize, clip, proc, **kw)
    cxcy = txt2img.generate(am, policy, pool, PROMPT, llm, tokenize, clip, proc, is_center=True, **kw)
    assert xywh["bboxes_ltrb"] == [[0.5, 0.5, 0.9, 0.7]] and cxcy["bboxes_ltrb"] == [[0.3, 0.4, 0.7, 0.6]]
    assert xywh["cids"] == [] and llm.seen[0] == build_prompt([], {"captions": PROMPT}) == llm.seen[1]
    assert not np.array_equal(np.asarray(xywh["images"][0]), np.asarray(cxcy["images"][0]))
    # every candidate as an example: shot_number above the pool's size yields the whole pool, best last
    allk = txt2img.generate(am, policy, pool, PROMPT, llm, tokenize, clip, proc, **{**kw, "shot_number": 32})
    assert allk["cids"] == fp64_cids(towers, pool, 32) and sorted(allk["cids"]) == list(range(6))


@pytest.mark.gpu
def test_generate_raises_on_an_answer_without_a_box(setup):
    am, clip, proc, towers, pool, policy = setup
    text = "I cannot help with cat: [1, 2, 3, 4]"
    with pytest.raises(ValueError) as e:
        txt2img.generate(am, policy, pool, PROMPT, StubLLM(text), tokenize, clip, proc, num_per_prompt=1, steps=4,
                         starting_noise=torch.zeros(1, 4, 16, 16), device=DEV)
    assert text in str(e.value)
    with pytest.raises(ValueError, match="starting_noise"):
        txt2img.generate(am, policy, pool, PROMPT, StubLLM(ANSWER), tokenize, clip, proc, num_per_prompt=2, starting_noise=torch.zeros(1, 4, 16, 16))


def test_generate_refuses_a_model_that_is_not_box_grounded_before_the_llm_is_called():
    """needs no GPU: the family is checked before anything runs"""
    llm = StubLLM(ANSWER)
    pool = CandidatePool(EXAMPLES, torch.zeros(6, 768))
    for family in ("keypoint", "spatial"):
        am = (types.SimpleNamespace(cfg=dataclasses.replace(TINY, grounding=family)), None, None, None, {})
        with pytest.raises(ValueError, match=family):
            txt2img.generate(am, PolicyNetwork(device="cpu"), pool, PROMPT, llm, tokenize)
    assert llm.seen == []
