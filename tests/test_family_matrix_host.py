"""CPU characterization of the grounding-family dispatch (no GPU): what ``interface.run_one_image`` / ``run_batch_images`` refuse, and with which
exception and message, for every family's valid meta plus every single and every pair of foreign meta keys; what the five grounding-input classes
return from ``prepare`` and ``get_null_input``; and the family each config belongs to.

The refusal expectations are ``tests/golden/family_refusals.json``, written by this module's own generator (``python
tests/test_family_matrix_host.py --write``) from the commit BEFORE the family record existed: the module uses only names that commit exports, and
it passes there unchanged."""
import dataclasses
import itertools
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # the generator runs from anywhere
import inpaint9_cases as ic
import kp_cases as kc
import sem_cases as sm
import sp_cases as sc
from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd.arch import TINY
from layoutllm_t2i_amd.model import (GroundingNetInput, KeypointGroundingNetInput, SemGroundingNetInput, SpatialGroundingNetInput,
                                     TextImageGroundingNetInput, grounding_input_for)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "family_refusals.json")
BOX = [0.1, 0.1, 0.5, 0.5]
PERSON = [[0.1 + 0.01 * i, 0.2] for i in range(17)]
FOREIGN = ("images", "input_image", "locations", "sem", "canny_image", "hed_image", "depth", "normal")
COMBOS = [c for n in (0, 1, 2) for c in itertools.combinations(FOREIGN, n)]          # 1 + 8 + 28, in this order in the golden file

# name -> (config, family, grounding-input class, the valid meta's own grounding keys)
CONFIGS = {
    "text": (TINY, "text", GroundingNetInput, dict(phrases=["a"], locations=[BOX])),
    "text_image": (dataclasses.replace(TINY, grounding="text_image"), "text_image", TextImageGroundingNetInput, dict(phrases=["a"], locations=[BOX])),
    "keypoint": (kc.KP_TINY[8], "keypoint", KeypointGroundingNetInput, dict(locations=[PERSON])),
    "canny": (sc.CANNY_TINY, "spatial", SpatialGroundingNetInput, dict(canny_image="a.png")),
    "hed": (sc.HED_TINY, "spatial", SpatialGroundingNetInput, dict(hed_image="a.png")),
    "sem": (sm.SEM_TINY, "sem", SemGroundingNetInput, dict(sem="a.png")),
    "inpaint": (ic.IP_TINY, "text", GroundingNetInput, dict(phrases=["a"], locations=[BOX], input_image="in.png")),
    "inpaint_without_image": (ic.IP_TINY, "text", GroundingNetInput, dict(phrases=["a"], locations=[BOX])),
    "norel": (dataclasses.replace(TINY, relation=False), "text", GroundingNetInput, dict(phrases=["a"], locations=[BOX])),
}


class _Past(Exception):
    """raised by the first thing ``_run`` touches after its last refusal"""


class _Config(dict):
    def update(self, *a, **k):
        raise _Past()


class _Model:
    """carries ``cfg`` alone: any other attribute ``_run`` reads before its last refusal is an AttributeError in the outcome"""

    def __init__(self, cfg):
        self.cfg = cfg


class _MapModel(_Model):
    def grounding_extra_of(self, input, hw=None):
        return None


def _meta(own, foreign, multiple):
    """the family's valid meta with the foreign keys laid over it, in the single or the one-layout-per-prompt form"""
    m = dict(own)
    for k in foreign:
        m[k] = {"images": ["b.png"], "locations": [BOX]}.get(k, k + ".png")
    if multiple:
        for k in ("phrases", "locations", "images"):
            if k in m:
                m[k] = [m[k]]
        if "input_image" in m:
            m["input_image"] = [m["input_image"]]
    return dict(m, **({"prompts": ["x"]} if multiple else {"prompt": "x"}))


def outcome(name, foreign, multiple):
    cfg, family, _, own = CONFIGS[name]
    model = (_MapModel if family in ("spatial", "sem") else _Model)(cfg)
    run = itf.run_batch_images if multiple else itf.run_one_image
    try:
        run((model, None, None, None, _Config()), dict(batch_size=1), _meta(own, foreign, multiple), torch.zeros(1, 4, 16, 16))
    except _Past:
        return None
    except Exception as ex:          # noqa: BLE001 -- the type is part of what is recorded
        return [type(ex).__name__, str(ex)]
    raise AssertionError("_run returned from a model that has nothing but a config")


def all_outcomes():
    """{"outcomes": the distinct [type, message] (null = got past the refusals), "cases": {"<config>/<one|batch>": index per COMBOS entry}}"""
    distinct, cases = [None], {}
    for name in CONFIGS:
        for multiple in (False, True):
            row = []
            for foreign in COMBOS:
                o = outcome(name, foreign, multiple)
                if o not in distinct:
                    distinct.append(o)
                row.append(distinct.index(o))
            cases[f"{name}/{'batch' if multiple else 'one'}"] = row
    return {"foreign": list(FOREIGN), "outcomes": distinct, "cases": cases}


# ------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name", list(CONFIGS))
def test_refusals_are_the_recorded_ones(name):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["foreign"] == list(FOREIGN) and all(len(r) == len(COMBOS) == 37 for r in gold["cases"].values())
    for multiple in (False, True):
        row = gold["cases"][f"{name}/{'batch' if multiple else 'one'}"]
        for foreign, idx in zip(COMBOS, row):
            assert outcome(name, foreign, multiple) == gold["outcomes"][idx], (name, multiple, foreign)


def test_the_valid_meta_gets_past_and_the_matrix_is_not_trivial():
    with open(GOLDEN) as f:
        gold = json.load(f)
    for name in CONFIGS:
        for form in ("one", "batch"):
            row = gold["cases"][f"{name}/{form}"]
            assert (row[0] == 0) == (name != "inpaint_without_image") and any(i != 0 for i in row)
    assert len(gold["outcomes"]) >= 12 and all(o is None or o[0] == "ValueError" for o in gold["outcomes"])


# ------------------------------------------------------------------------------------------- grounding inputs
def _batches():
    f = lambda *s: torch.rand(*s)
    return {
        GroundingNetInput: dict(boxes=f(2, 30, 4), masks=f(2, 30), text_embeddings=f(2, 30, 768)),
        TextImageGroundingNetInput: dict(boxes=f(2, 30, 4), masks=f(2, 30), text_masks=f(2, 30), image_masks=f(2, 30),
                                         text_embeddings=f(2, 30, 768), image_embeddings=f(2, 30, 768)),
        KeypointGroundingNetInput: dict(points=f(2, 51, 2), masks=f(2, 51)),
        SpatialGroundingNetInput: dict(map=f(2, 3, 32, 32), mask=torch.ones(2, 1)),
        SemGroundingNetInput: dict(sem=torch.zeros(2, 32, 32, dtype=torch.uint8), mask=torch.ones(2, 1)),
    }


F32, U8 = torch.float32, torch.uint8
# class -> {key: (shape behind the batch axis, dtype)} of get_null_input() after prepare(_batches()[class])
NULLS = {
    GroundingNetInput: {"boxes": ((30, 4), F32), "masks": ((30,), F32), "positive_embeddings": ((30, 768), F32)},
    TextImageGroundingNetInput: {"boxes": ((30, 4), F32), "masks": ((30,), F32), "text_masks": ((30,), F32), "image_masks": ((30,), F32),
                                 "text_embeddings": ((30, 768), F32), "image_embeddings": ((30, 768), F32)},
    KeypointGroundingNetInput: {"points": ((51, 2), F32), "masks": ((51,), F32)},
    SpatialGroundingNetInput: {"map": ((3, 32, 32), F32), "mask": ((), F32)},
    SemGroundingNetInput: {"sem": ((32, 32), U8), "mask": ((), F32)},          # the class map keeps its dtype, the mask is float32
}


@pytest.mark.parametrize("cls", list(NULLS), ids=[c.__name__ for c in NULLS])
def test_grounding_input_contract(cls):
    g, batch = cls(), _batches()[cls]
    with pytest.raises(AssertionError, match="^not set yet, cannot call this funcion$"):
        g.get_null_input()
    out = g.prepare(batch, None)                        # the two-argument call of the interface
    assert set(out) == set(NULLS[cls]) and g.prepare(batch).keys() == out.keys()
    for k, v in out.items():
        assert v is batch["text_embeddings" if k == "positive_embeddings" else k]
    for n, null in ((2, g.get_null_input()), (3, g.get_null_input(batch=3))):
        assert {k: (tuple(v.shape), v.dtype) for k, v in null.items()} == {k: ((n,) + s, d) for k, (s, d) in NULLS[cls].items()}
        assert list(null) == list(out) and all(float(v.float().abs().max()) == 0.0 for v in null.values())
    half = g.get_null_input(dtype=torch.float16)
    assert {k: v.dtype for k, v in half.items()} == {k: (F32 if (cls is SemGroundingNetInput and k == "mask") else torch.float16) for k in half}
    if cls is KeypointGroundingNetInput:
        assert g.max_persons_per_image == 3 and isinstance(g.max_persons_per_image, int)


def test_text_input_builds_embeddings_from_labels():
    class _Enc:
        def __init__(self):
            self.seen = []

        def encode_one_token(self, label):
            self.seen.append(label)
            return torch.full((768,), float(len(self.seen)))
    enc, g = _Enc(), GroundingNetInput()
    masks = torch.zeros(2, 30)
    masks[0, :2], masks[1, :1] = 1, 1
    out = g.prepare(dict(boxes=torch.rand(2, 30, 4), masks=masks, labels=["cat|dog|unused", "tree"]), enc)
    assert enc.seen == ["cat", "dog", "tree"] and list(out) == ["boxes", "masks", "positive_embeddings"]
    pe = out["positive_embeddings"]
    assert tuple(pe.shape) == (2, 30, 768) and pe[0, 0, 0] == 1 and pe[0, 1, 5] == 2 and pe[1, 0, 767] == 3 and float(pe[0, 2:].abs().max()) == 0
    assert float(pe[1, 1:].abs().max()) == 0 and tuple(g.get_null_input()["positive_embeddings"].shape) == (2, 30, 768)


# ------------------------------------------------------------------------------------------- the family of each config
@pytest.mark.parametrize("name", list(CONFIGS))
def test_each_config_has_its_family(name):
    cfg, family, cls, _ = CONFIGS[name]
    assert type(grounding_input_for(cfg)) is cls                     # sem is told from canny, though both are grounding == "spatial"
    try:
        from layoutllm_t2i_amd.family import family_of
    except ImportError:
        pytest.skip("the commit this module characterizes has no family record yet")
    assert family_of(cfg).name == family and family_of(_Model(cfg).cfg) is family_of(cfg)
    assert set(family_of(cfg).keys) == set(NULLS[cls])


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_family_matrix_host.py --write      (regenerates tests/golden/family_refusals.json)")
    with open(GOLDEN, "w") as f:
        json.dump(all_outcomes(), f, indent=0)
        f.write("\n")
