"""The prompt-to-image entry of LayoutLLM-T2I (the reference's ``generate``, txt2img.py:460-508): a prompt, a trained policy and a pool
of candidate layouts in, images out.

    1. embed the prompt with the CLIP text tower the pool was embedded with          txt2img.py:463-464
    2. policy.select: the shot_number best candidates, most relevant last (device)    :472-474, :429-431
    3. prompting.build_prompt: the LLM prompt with these in-context examples          :434
    4. llm(prompt_text) -> str: ANY callable the caller supplies                      :443
    5. prompting.extract_prediction: ``object: [x, y, w, h]`` lines                   :445
    6. boxes -> (left, top, right, bottom)                                            :487-491
    7. interface.run_one_image in batches until num_per_prompt images exist           :499-508

There is no network code here and no API client: ``llm`` is the caller's.  Deviations from the reference, all deliberate:
an answer without one parsable box raises ValueError (the reference would generate from an empty layout); only the box-grounded
checkpoint families run (text, text_image without reference images): a keypoint / spatial / semantic-map model raises ValueError
before anything runs; images are generated ``batch_size`` at a time (the reference: one call per image).
"""
from __future__ import annotations

import os
from typing import Callable, Optional, Sequence

import torch

from . import interface
from .family import FAMILIES, family_of
from .policy import CandidatePool, PolicyNetwork, embed_texts
from .prompting import build_prompt, convert_xcycwh_to_ltrb, convert_xywh_to_ltrb, extract_prediction
from .sampler import DEFAULT_SAMPLER

BOX_FAMILIES = tuple(f.name for f in FAMILIES.values() if f.boxes)


def _save(images, folder: str, prompt: str, locations, phrases, draw_boxes: bool) -> None:
    """``{prompt}_{i}.jpg`` under ``folder`` (txt2img.py:497-507); ``draw_boxes``: the layout drawn over the saved copy"""
    os.makedirs(folder, exist_ok=True)
    for i, im in enumerate(images):
        if draw_boxes:
            from PIL import ImageDraw
            im = im.copy()
            d = ImageDraw.Draw(im)
            W, H = im.size
            for (l, t, r, b), name in zip(locations, phrases):
                d.rectangle([l * W, t * H, r * W, b * H], outline=(255, 0, 0), width=2)
                d.text((l * W + 3, t * H + 3), name, fill=(255, 0, 0))
        im.save(os.path.join(folder, f"{prompt}_{i}.jpg"))


def generate(all_models, policy: PolicyNetwork, pool: CandidatePool, prompt: str, llm: Callable[[str], str], tokenize: Callable,
             clip_model=None, clip_processor=None, shot_number: int = 2, num_per_prompt: int = 5, batch_size: int = 1,
             guidance_scale: float = 7.5, alpha_type: Sequence[float] = (0.3, 0.0, 0.7), is_center: bool = False,
             steps: Optional[int] = None, starting_noise: Optional[torch.Tensor] = None, folder: Optional[str] = None, device=None,
             instruction=None, draw_boxes: bool = False, sampler: str = "plms", ddim_eta: float = 0.0, dpm_order: int = 2,
             dpm_discretize: str = "logsnr", layout_guidance_scale: Optional[float] = None, init_image=None,
             strength: Optional[float] = None) -> dict:
    """``all_models``: the 5-tuple of ``interface.load_all_models``; ``policy`` / ``pool``: policy.PolicyNetwork / policy.CandidatePool;
    ``tokenize``: list of strings -> (input_ids, attention_mask) for the CLIP text tower (``pool.towers``, else ``clip_model``);
    ``clip_model`` / ``clip_processor``: the grounding phrases' encoder, as for ``interface.generate_one_image``.
    ``is_center``: the LLM's boxes are [xc, yc, w, h], not [x, y, w, h].  ``steps``: handed through as ``args["steps"]`` (None: the
    reference's 50).  ``starting_noise``: [num_per_prompt, 4, h, w], row i for image i; None: ``torch.randn(n, 4, 64, 64)`` from the global
    CPU generator per batch, as ``generate_one_image`` draws it.  ``folder``: save ``{prompt}_{i}.jpg`` there (``draw_boxes``: with the
    layout drawn on the saved copies).  ``instruction``: the wording of the LLM prompt (prompting.build_prompt).  ``sampler`` / ``ddim_eta``:
    handed through as ``args["sampler"]`` / ``args["ddim_eta"]`` ("ddim" with eta >= 0; checked before the policy or the LLM runs);
    ``dpm_order`` / ``dpm_discretize``: ``args["dpm_order"]`` / ``args["dpm_discretize"]`` of ``sampler="dpmpp_2m"`` (sampler.resolve_sampler;
    with ``steps=20`` an image costs 20 UNet evaluations in place of PLMS's 51).  ``layout_guidance_scale``: None, or how hard the images
    follow the LLM's boxes, apart from ``guidance_scale``'s prompt adherence -- ``args["layout_guidance_scale"]``
    (interface.check_layout_guidance; checked before the policy or the LLM runs).  ``init_image`` (a path or a PIL.Image) with ``strength``
    in (0, 1] (None: 0.75): image-to-image -- every image is that picture re-rendered under the prompt and the LLM's boxes, handed through
    as ``meta["init_image"]`` / ``args["strength"]`` (interface.check_strength; checked before the policy or the LLM runs).
    Returns dict(images, categories, bboxes_ltrb, cids, prompt_text, llm_output)."""
    model = all_models[0]
    if not family_of(model.cfg).boxes:
        raise ValueError(f"the prompt-to-image entry generates from boxes: a {model.cfg.grounding} checkpoint cannot run it "
                         f"(box-grounded families: {BOX_FAMILIES})")
    if num_per_prompt < 1 or batch_size < 1:
        raise ValueError(f"num_per_prompt = {num_per_prompt}, batch_size = {batch_size}: both must be >= 1")
    if starting_noise is not None and (starting_noise.dim() != 4 or starting_noise.shape[0] != num_per_prompt):
        raise ValueError(f"starting_noise {tuple(starting_noise.shape)}: expected [num_per_prompt = {num_per_prompt}, 4, h, w]")
    given = dict(sampler=sampler, ddim_eta=ddim_eta, dpm_order=dpm_order, dpm_discretize=dpm_discretize)
    spec, values = interface.resolve_sampler(given)
    # handed on: nothing for the default sampler, else the sampler and those of its own keys this entry takes
    sampler_args = {} if spec.name == DEFAULT_SAMPLER else {k: values[k] for k in ("sampler", *(key.name for key in spec.keys)) if k in given}
    layout = interface.check_layout_guidance(layout_guidance_scale, family_of(model.cfg))
    if layout is not None:
        sampler_args[interface.LAYOUT_GUIDANCE_KEY] = layout
    strength = interface.check_strength(strength, init_image is not None)
    if strength is not None:
        sampler_args[interface.STRENGTH_KEY] = strength
    towers = pool.towers if pool.towers is not None else clip_model
    if towers is None:
        raise ValueError("no text tower for the prompt: build the pool with CandidatePool.from_captions, or pass clip_model")
    device = policy.device if device is None else device

    emb_prompt = embed_texts(towers, tokenize, [prompt])
    cids = policy.select(emb_prompt, pool.features, shot_number)[0].tolist()
    shot_cand = [pool.examples[c] for c in cids]
    prompt_text = build_prompt(shot_cand, {"captions": prompt}, instruction)
    output = llm(prompt_text)
    if not isinstance(output, str):
        raise TypeError(f"llm returned {type(output).__name__}, expected the answer as a string")
    categories, bboxes = extract_prediction(output)
    if not bboxes:
        raise ValueError(f"the LLM's answer holds no 'object: [x, y, w, h]' item; the answer was: {output!r}")
    convert = convert_xcycwh_to_ltrb if is_center else convert_xywh_to_ltrb
    locations = [convert(b) for b in bboxes]
    meta = dict(prompt=prompt, phrases=categories, locations=locations, alpha_type=list(alpha_type))
    if init_image is not None:
        meta[interface.INIT_IMAGE_KEY] = init_image

    images = []
    h, w = interface.latent_hw(None, None, all_models[1]) if starting_noise is None else (0, 0)
    while len(images) < num_per_prompt:
        n = min(batch_size, num_per_prompt - len(images))
        args = dict(batch_size=n, no_plms=False, guidance_scale=guidance_scale)
        args.update(sampler_args)
        if steps is not None:
            args["steps"] = int(steps)
        noise = torch.randn(n, 4, h, w) if starting_noise is None else starting_noise[len(images):len(images) + n]
        images += interface.run_one_image(all_models, args, meta, noise.to(device), clip_model, clip_processor, device=device)
    if folder is not None:
        _save(images, folder, prompt, locations, categories, draw_boxes)
    return dict(images=images, categories=categories, bboxes_ltrb=locations, cids=cids, prompt_text=prompt_text, llm_output=output)
