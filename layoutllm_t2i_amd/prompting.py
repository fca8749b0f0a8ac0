"""Host-side text work of the prompt-to-image entry: the LLM prompt with its in-context examples, and the parser of the LLM's answer.

    build_prompt(shot_cand, example, instruction=None)     the layout of base_prompt.py:22-45
    extract_prediction(text) -> (categories, bboxes)       utils.py:78-93
    center2lefttop(boxes)                                  utils.py:95-101
    convert_xywh_to_ltrb / convert_xcycwh_to_ltrb          interface.py (re-exported)

The LAYOUT of the prompt is the reference's: a preamble, one block per in-context example (its caption, then one ``label: [x, y, w, h]``
line per box, centre boxes moved to their top-left corner and rounded to 2 places), and the query line.  The WORDING the LLM reads -- the
task preamble and the note behind the query -- is an argument: ``instruction``.  Its default is this project's own description of the
task; a caller who wants the reference's exact prompt passes its wording (tests/golden/prompting_ref.json records it as data, and with it
``build_prompt`` reproduces the reference's prompt character for character).
"""
from __future__ import annotations

import re
from typing import Mapping, Optional, Sequence, Union

from .interface import convert_xcycwh_to_ltrb, convert_xywh_to_ltrb  # noqa: F401  (re-exported)

# this project's wording: what a layout is, the box format with its range, and the answer format the parser reads
_TASK = ("You design image layouts. Given a description of an image, list the objects it should show, one per line, as "
         "\"name: [x, y, w, h]\". The name is a short object name of one or two words. x and y are the top left corner of the "
         "object's bounding box, w its width and h its height, each written as a decimal fraction of the image size, so that "
         "x, y, w, h, x+w and y+h all lie between 0 and 1. ")
DEFAULT_INSTRUCTION = {
    "few_shot": _TASK + "Some descriptions with their layouts follow; answer the last description in the same form.",
    "zero_shot": _TASK + "A description follows. Answer in this form:\noutput:\nname: [x, y, w, h]\nname: [x, y, w, h]\n...",
    "query_note": " (Answer with the layout only, without comments. If the description leaves things open, choose a plausible layout.)",
}


def _wording(instruction, few_shot: bool):
    """-> (preamble, query note) for ``instruction``: None (the default wording), a string (the preamble for both forms, default
    note) or a mapping with any of ``few_shot`` / ``zero_shot`` / ``query_note``"""
    if instruction is None:
        instruction = DEFAULT_INSTRUCTION
    if isinstance(instruction, str):
        return instruction, DEFAULT_INSTRUCTION["query_note"]
    unknown = set(instruction) - set(DEFAULT_INSTRUCTION)
    if unknown:
        raise ValueError(f"instruction keys {sorted(unknown)}: expected {sorted(DEFAULT_INSTRUCTION)}")
    key = "few_shot" if few_shot else "zero_shot"
    return instruction.get(key, DEFAULT_INSTRUCTION[key]), instruction.get("query_note", DEFAULT_INSTRUCTION["query_note"])


def build_prompt(shot_cand: Sequence[Mapping], example: Mapping, instruction: Union[None, str, Mapping[str, str]] = None) -> str:
    """The LLM prompt for ``example['captions']`` with the in-context examples ``shot_cand`` (records with ``captions``, ``label``
    and ``bbox`` = centre boxes [xc, yc, w, h]), laid out as base_prompt.py:22-45 does; no example: the zero-shot form."""
    blocks = []
    for cand in shot_cand:
        lines = ["output: "]
        for jj, label in enumerate(cand["label"]):
            xc, yc, w, h = cand["bbox"][jj]
            box = [round(v, 2) for v in (xc - w / 2, yc - h / 2, w, h)]
            lines.append(label + ": " + str(box))
        blocks.append("\ninput: " + cand["captions"] + "\n" + "\n".join(lines) + "\n")
    context = "".join(blocks)
    preamble, note = _wording(instruction, bool(context))
    return preamble + "\n" + context + "\n" + "input: " + example["captions"] + note


_NUMBER = r"(\d+\.\d+)"
# a name of one word, or two with any space between (of a longer name the last two words), a colon, four decimals in brackets
_ITEM = re.compile(r"\b(\w+\s*\w*)\s*:\s*\[" + r",\s*".join([_NUMBER] * 4) + r"\]")


def extract_prediction(text: str):
    """``name: [x, y, w, h]`` items of an LLM answer -> (names, boxes of four floats), in order of appearance, exactly as
    utils.py:78-93 reads them: a number needs a decimal point and no sign (an item with ``1`` or ``-0.1`` is skipped), of a name
    with more than two words the last two survive, several items may share a line; no item: two empty lists."""
    names, boxes = [], []
    for m in _ITEM.findall(text):
        names.append(m[0])
        boxes.append([float(v) for v in m[1:5]])
    return names, boxes


def center2lefttop(boxes):
    """[xc, yc, w, h] -> [x, y, w, h] per box (utils.py:95-101)"""
    return [[xc - w / 2, yc - h / 2, w, h] for xc, yc, w, h in boxes]
