"""The policy-gradient trainer of LayoutLLM-T2I (the reference's train_rl.py) with the outside world injected: ``train_batch`` is its
``get_batch_reward_loss`` (:23-98) plus the update (:182-184), ``policy_gradient_train`` its epoch loop (:116-257) with the same files.

    per batch   probabilities (device) -> per row: sample_examples, build_prompt, llm(text), extract_prediction; a row whose answer
                holds no box is dropped -> generate(captions, categories, bboxes) -> reward(...) -> PolicyTrainer.step on the kept rows
    per epoch   ckpt_{epoch}.pt (the layer), state_{epoch}.pt (Adam and StepLR), ckpt_best_reward.pt / ckpt_best_loss.pt, history.json,
                PolicyTrainer.epoch_end; at the end ckpt_final.pt

``llm`` is the caller's callable (text -> answer), as in ``txt2img.generate``; ``generate`` and ``reward`` are callables too, with
ready-made adaptors for the package's own pipeline (``generate_with``, ``reward_with``).  There is no logger, no progress bar, no argument
parser and no network code here.
"""
from __future__ import annotations

import json
import math
import os
from typing import Callable, Mapping, Optional, Sequence

import numpy as np
import torch

from .policy import CandidatePool, sample_examples
from .policy_train import PolicyTrainer
from .prompting import build_prompt, center2lefttop, extract_prediction


def generate_with(all_models, clip_model=None, clip_processor=None, device=None, sampler=None, steps=None, dpm_order=None,
                  dpm_discretize=None, layout_guidance_scale=None) -> Callable:
    """``generate`` for ``train_batch``: ``interface.generate_batch_images`` on ``all_models`` (train_rl.py:90-91).  ``sampler`` / ``steps`` /
    ``dpm_order`` / ``dpm_discretize``: when any is given, the same call through ``interface.run_batch_images`` with those as ``args`` keys
    (the rollout images only feed the reward: ``sampler="dpmpp_2m", steps=20`` is 20 UNet evaluations per image in place of 51); checked
    here, before the rollout.  ``layout_guidance_scale``: the layout's own guidance scale (interface.check_layout_guidance), routed the same
    way -- how hard the rollout follows the LLM's boxes, without touching prompt adherence.  None given: ``generate_batch_images`` exactly."""
    from . import interface
    from .family import family_of
    more = {k: v for k, v in dict(sampler=sampler, steps=steps, dpm_order=dpm_order, dpm_discretize=dpm_discretize).items() if v is not None}
    if more:
        interface.resolve_sampler(more)         # every key of the switch that was given, judged the way the rollout's call will judge it
    if layout_guidance_scale is not None:
        more[interface.LAYOUT_GUIDANCE_KEY] = interface.check_layout_guidance(layout_guidance_scale, family_of(getattr(all_models[0], "cfg", None)))

    def generate(captions, categories, bboxes):
        if not more:
            return interface.generate_batch_images(all_models, captions, categories, bboxes, clip_model, clip_processor, device)
        # generate_batch_images' own call (its 512 x 512 images, its starting-noise draw), with the per-call keys added
        h, w = interface.latent_hw(None, None, all_models[1])
        bs = len(captions)
        args = dict(batch_size=bs, no_plms=False, guidance_scale=7.5, **more)
        meta = dict(prompts=captions, phrases=categories, locations=bboxes, alpha_type=[0.3, 0.0, 0.7])
        starting_noise = torch.randn(bs, 4, h, w).to(device)
        return interface.run_batch_images(all_models, args, meta, starting_noise, clip_model, clip_processor, device=device)
    return generate


def reward_with(reward_model, tokenize: Callable) -> Callable:
    """``reward`` for ``train_batch``: ``reward.RewardModel.forward_layouts`` (train_rl.py:93), the ground-truth centre boxes turned into
    [x, y, w, h] first (train_rl.py:83); ``tokenize``: list of strings -> (input_ids, attention_mask).  Returns the reward as double."""
    def reward(captions, images_pred, images_gt, layout_pred, layout_gt):
        ids, mask = tokenize(list(captions))
        gt = [(center2lefttop(boxes), labels) for boxes, labels in layout_gt]
        out = reward_model.forward_layouts(ids, images_pred, images_gt, layout_pred, gt, tokenize, attention_mask=mask)
        return out["reward"].to(torch.float64)
    return reward


def train_batch(trainer: PolicyTrainer, pool: CandidatePool, batch: Sequence[Mapping], emb_batch, llm: Callable[[str], str],
                generate: Callable, reward: Callable, shot_number: int = 2, temperature: float = 1.0, rng=np.random, instruction=None) -> dict:
    """One rollout batch and one update.  ``batch``: the training records (``captions``, ``label``, ``bbox`` = centre boxes, optionally
    ``image``: the ground-truth image); ``emb_batch``: their CLIP text features [B, D].  Per row, in order: the probabilities' row is drawn
    from with ``sample_examples`` (numpy's stream ``rng``), the prompt is built from the drawn examples (most relevant last), ``llm``
    answers, the answer is parsed; a row without one parsable box is dropped (the reference's ``continue``, train_rl.py:75-76).
    ``generate(captions, categories, bboxes)`` -> images; ``reward(captions, images_pred, images_gt, layout_pred, layout_gt)`` -> [kept]
    floats, a device tensor (``layout_pred``: (boxes, names) per row; ``layout_gt``: the record's (bbox, label)).  ``trainer.step`` then
    takes the kept rows with the drawn pool indices in drawn order (un-reversed) as ``sel``.
    Returns ``dict(reward, loss, cids, kept)``: the batch's summed reward and its loss as floats (the one host read of the loss), the
    last row's prompt order of examples, and the indices of the rows that were kept.  All rows dropped: no step, reward 0, loss 0."""
    if len(batch) < 1:
        raise ValueError("an empty batch")
    emb_batch = torch.as_tensor(emb_batch)
    if emb_batch.dim() != 2 or emb_batch.shape[0] != len(batch):
        raise ValueError(f"{len(batch)} records but emb_batch {tuple(emb_batch.shape)}")
    probs = trainer.policy.probabilities(emb_batch, pool.features, temperature).cpu()
    kept, sel, captions, images_gt, layout_pred, layout_gt = [], [], [], [], [], []
    cids = np.zeros(0, np.int64)
    for i, ex in enumerate(batch):
        cids = sample_examples(probs[i], shot_number, rng)
        text = build_prompt([pool.examples[c] for c in cids], ex, instruction)
        answer = llm(text)
        if not isinstance(answer, str):
            raise TypeError(f"llm returned {type(answer).__name__}, expected the answer as a string")
        categories, bboxes = extract_prediction(answer)
        if len(categories) == 0:
            continue
        kept.append(i)
        sel.append(np.asarray(cids[::-1], np.int64))
        captions.append(ex["captions"])
        images_gt.append(ex.get("image"))
        layout_pred.append((bboxes, categories))
        layout_gt.append((ex["bbox"], ex["label"]))
    if not kept:
        return dict(reward=0.0, loss=0.0, cids=cids.tolist(), kept=[])
    images = generate(captions, [c for _, c in layout_pred], [b for b, _ in layout_pred])
    r = torch.as_tensor(reward(captions, images, images_gt, layout_pred, layout_gt))
    if tuple(r.shape) != (len(kept),):
        raise ValueError(f"reward returned {tuple(r.shape)}, expected [{len(kept)}]")
    out = trainer.step(emb_batch[kept], pool.features, np.stack(sel), r, temperature)
    return dict(reward=float(r.sum()), loss=float(out["loss"]), cids=cids.tolist(), kept=kept)


def _latest_state(folder: str) -> int:
    """the highest epoch with a state_{epoch}.pt under ``folder`` (train_rl.py:100-107)"""
    epochs = [int(f[len("state_"):-len(".pt")]) for f in os.listdir(folder) if f.startswith("state_") and f.endswith(".pt") and f[len("state_"):-len(".pt")].isdigit()]
    if not epochs:
        raise FileNotFoundError(f"no state_*.pt under {folder}")
    return max(epochs)


def resume_from(trainer: PolicyTrainer, folder: str) -> int:
    """Loads ``ckpt_{n}.pt`` into the policy and ``state_{n}.pt`` into the trainer for the highest n under ``folder`` (train_rl.py:100-113;
    files of the reference load as well) and returns n."""
    n = _latest_state(folder)
    trainer.policy.load_state_dict(torch.load(os.path.join(folder, f"ckpt_{n}.pt"), map_location="cpu", weights_only=True))
    trainer.load_state_dict(torch.load(os.path.join(folder, f"state_{n}.pt"), map_location="cpu", weights_only=True))
    return n


def policy_gradient_train(trainer: PolicyTrainer, pool: CandidatePool, train_examples: Sequence[Mapping], emb_train, llm: Callable[[str], str],
                          generate: Callable, reward: Callable, ckpt_path: str, epochs: int, batch_size: int, resume: str = "",
                          new_lr: Optional[float] = None, shot_number: int = 2, temperature: float = 1.0, rng=np.random,
                          instruction=None) -> dict:
    """The epoch loop of train_rl.py:116-257: ``epochs`` passes over ``train_examples`` (``emb_train``: their features [n, D]) in batches of
    ``batch_size``, in order.  ``resume``: a folder of an earlier run; training continues after its highest ``state_{epoch}.pt`` with that
    run's Adam state, step count and learning rate; ``new_lr``: the reference's "use new learning rate" (``PolicyTrainer.set_lr``), which
    the reference applies on every start.  A NaN loss ends the run after that epoch's files are written.
    Returns the history dict of ``history.json`` plus ``start_epoch`` and ``last_epoch``."""
    if epochs < 1 or batch_size < 1:
        raise ValueError(f"epochs = {epochs}, batch_size = {batch_size}: both must be >= 1")
    emb_train = torch.as_tensor(emb_train)
    if emb_train.dim() != 2 or emb_train.shape[0] != len(train_examples) or len(train_examples) < 1:
        raise ValueError(f"{len(train_examples)} training records but emb_train {tuple(emb_train.shape)}")
    os.makedirs(ckpt_path, exist_ok=True)
    start_epoch = 0
    if resume:
        start_epoch = resume_from(trainer, resume) + 1
        trainer.epoch_end()          # state_{epoch}.pt is written before that epoch's scheduler step (train_rl.py:221, :250): take it now
    if new_lr is not None:
        trainer.set_lr(new_lr)
    history = dict(reward_history=[], loss_history=[], total_reward_history=[], total_loss_history=[])
    save = lambda name: torch.save(trainer.weights(), os.path.join(ckpt_path, name))
    epoch = start_epoch
    for epoch in range(start_epoch, start_epoch + epochs):
        total_reward = total_loss = 0.0
        stop = False
        for lo in range(0, len(train_examples), batch_size):
            res = train_batch(trainer, pool, train_examples[lo:lo + batch_size], emb_train[lo:lo + batch_size], llm, generate, reward,
                              shot_number, temperature, rng, instruction)
            total_reward += res["reward"]
            total_loss += res["loss"]
            history["reward_history"].append(res["reward"])
            history["loss_history"].append(res["loss"])
            if math.isnan(res["loss"]):
                stop = True
                break
        history["total_reward_history"].append(total_reward)
        history["total_loss_history"].append(total_loss)
        best_reward_epoch = history["total_reward_history"].index(max(history["total_reward_history"])) + start_epoch
        best_loss_epoch = history["total_loss_history"].index(min(history["total_loss_history"])) + start_epoch
        save(f"ckpt_{epoch}.pt")
        torch.save(trainer.state_dict(), os.path.join(ckpt_path, f"state_{epoch}.pt"))
        if epoch == best_reward_epoch:
            save("ckpt_best_reward.pt")
        if epoch == best_loss_epoch:
            save("ckpt_best_loss.pt")
        with open(os.path.join(ckpt_path, "history.json"), "w") as f:
            json.dump(history, f, indent=2, separators=(",", ": "))
        trainer.epoch_end()
        if stop:
            break
    save("ckpt_final.pt")
    return dict(history, start_epoch=start_epoch, last_epoch=epoch)
