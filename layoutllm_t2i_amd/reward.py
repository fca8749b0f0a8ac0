"""Reward scoring stage of the train_rl.py rollout on the MI355X (BASELINE.json configs[4]).

Mirrors the GPU part of ``Reward_Model.forward`` (models/policy.py:106-135): CLIP text-image / image-image cosine
similarities and the AestheticMLP score (tools/aesthetic.py:15-31) run in ONE HIP kernel (``gl_reward_score``) on the
CLIP features of the rollout batch; ``reward = clip + 0.1 * aes + 10 * mIoU + 10 * DocSim`` (policy.py:135) is finished
on the host with the layout terms, which are passed in.  Those two terms, which the reference computes in CPU python
(``compute_maximum_iou`` / ``compute_docsim``, tools/metrics.py), have their own kernel (``gl_layout_reward``, one wave per
sample and term) behind ``layout_terms``; ``RewardModel.forward_layouts`` runs policy.py:126-135 with it, the nearest-label
step (``nn_close_set``) on the HIP text tower.  ``RewardModel`` adds the CLIP towers (``clip.ClipTowers``: get_text_features / get_image_features of
the reference's transformers.CLIPModel on the HIP kernels), i.e. the whole GPU part of ``Reward_Model.forward``; the
tokenizer and the image processor (PIL resize / crop / normalise) stay the caller's CPU objects, as in the reference.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import LayoutRewardArgs, RewardArgs, check

F32 = torch.float32
# nn.Sequential indices of the five Linear layers of AestheticMLP (tools/aesthetic.py:21-34; Dropouts sit in between)
_LINEARS = (0, 2, 4, 6, 7)
_SHAPES = ((1024, None), (128, 1024), (64, 128), (16, 64), (1, 16))


MAX_BOXES = 64       # GL_LAYOUT_MAX_BOXES: one lane of the kernel's wave per box
# the closed label set of Reward.emb_labels (models/policy.py:56-64; COCO's 80 names): the ORDER decides the label ids
COCO_LABELS = (
    "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
    "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow",
    "elephant", "bear", "zebra", "giraffe", "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee",
    "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard",
    "tennis racket", "bottle", "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple",
    "sandwich", "orange", "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch",
    "potted plant", "bed", "dining table", "toilet", "tv", "laptop", "mouse", "remote", "keyboard",
    "cell phone", "microwave", "oven", "toaster", "sink", "refrigerator", "book", "clock", "vase", "scissors",
    "teddy bear", "hair drier", "toothbrush")


def pack_layouts(layouts: Sequence) -> tuple:
    """[(boxes [n, 4], label ids [n])] * B -> (boxes float64 [B, 64, 4], labels int32 [B, 64], counts int32 [B]) numpy arrays, zero padded.
    ValueError for more than 64 boxes, a box array that is not [n, 4] and a label array that is not [n]."""
    B = len(layouts)
    boxes, labels, counts = np.zeros((B, MAX_BOXES, 4), np.float64), np.zeros((B, MAX_BOXES), np.int32), np.zeros(B, np.int32)
    for b, (bx, lb) in enumerate(layouts):
        bx, lb = np.asarray(bx, dtype=np.float64), np.asarray(lb)
        n = int(lb.shape[0]) if lb.ndim == 1 else -1
        if n == 0 and bx.size == 0:
            continue                                   # np.array([]) of an empty layout is [0], not [0, 4]
        if bx.ndim != 2 or bx.shape[1] != 4:
            raise ValueError(f"layout {b}: boxes {tuple(bx.shape)}, expected [n, 4]")
        if n != bx.shape[0]:
            raise ValueError(f"layout {b}: {bx.shape[0]} boxes but labels {tuple(lb.shape)}")
        if n > MAX_BOXES:
            raise ValueError(f"layout {b}: {n} boxes, at most {MAX_BOXES} per layout")
        boxes[b, :n], labels[b, :n], counts[b] = bx, lb.astype(np.int32), n
    return boxes, labels, counts


def layout_terms(layout_gt: Sequence, layout_pred: Sequence, device="cuda:0") -> dict:
    """``compute_maximum_iou(layout_gt, layout_pred)`` and ``compute_docsim(layout_gt, layout_pred)`` (tools/metrics.py:58-164; policy.py:130-134)
    on the GPU: layouts are lists of (boxes [n, 4], label ids [n]) as ``label_to_id`` produces them.  Returns dict(miou, laysim) of float64 [B]
    device tensors, stream-ordered on the current stream, without a host synchronisation.  A sample whose IoU matrix holds 0/0 (two zero-area
    boxes) gets NaN where the reference raises.  ValueError: lists of different lengths, an empty list, an empty ground-truth layout (the
    reference: ZeroDivisionError), and what ``pack_layouts`` refuses.  The counts go to the library twice, as device arrays for the kernel and
    as host arrays it validates before the launch."""
    if len(layout_gt) != len(layout_pred):
        raise ValueError(f"{len(layout_gt)} ground-truth layouts but {len(layout_pred)} predicted ones")
    B = len(layout_gt)
    if B < 1:
        raise ValueError("no layouts")
    bg, lg, ng = pack_layouts(layout_gt)
    bp, lp, npd = pack_layouts(layout_pred)
    if (ng == 0).any():
        raise ValueError(f"layout {int(np.argmin(ng != 0))}: empty ground-truth layout (maximum IoU divides by its box count)")
    device = torch.device(device)
    # two copies: the doubles, the integers ([labels_gt | labels_pred | n_gt | n_pred])
    # from pinned staging tensors, so that the asynchronous copies are safe (the host allocator keeps a block until its copy is done)
    fh = torch.empty(2, B, MAX_BOXES, 4, dtype=torch.float64, pin_memory=True)
    ih = torch.empty(2 * B * MAX_BOXES + 2 * B, dtype=torch.int32, pin_memory=True)
    np.stack([bg, bp], out=fh.numpy())
    np.concatenate([lg.ravel(), lp.ravel(), ng, npd], out=ih.numpy())
    fd = fh.to(device, non_blocking=True)
    idv = ih.to(device, non_blocking=True)
    out = torch.empty(2, B, dtype=torch.float64, device=device)
    a = LayoutRewardArgs()
    a.boxes_gt, a.boxes_pred = fd[0].data_ptr(), fd[1].data_ptr()
    L = B * MAX_BOXES
    a.labels_gt, a.labels_pred = idv[:L].data_ptr(), idv[L:2 * L].data_ptr()
    a.n_gt, a.n_pred = idv[2 * L:2 * L + B].data_ptr(), idv[2 * L + B:].data_ptr()
    a.n_gt_host, a.n_pred_host = ng.ctypes.data, npd.ctypes.data
    a.B = B
    a.miou, a.docsim = out[0].data_ptr(), out[1].data_ptr()
    with torch.cuda.device(device):
        rc = _lib.lib().gl_layout_reward(C.byref(a), torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        raise _lib.HipLibraryError(f"gl_layout_reward failed with code {rc}: {_lib.last_error(None)}")
    return dict(miou=out[0], laysim=out[1])


class RewardScorer:
    def __init__(self, aesthetic_state_dict: Mapping[str, torch.Tensor], device="cuda:0", input_size: int = 768):
        """``aesthetic_state_dict``: the AestheticMLP checkpoint (keys ``layers.{0,2,4,6,7}.{weight,bias}``,
        models/policy.py:44-46 loads ``sac+logos+ava1-l14-linearMSE.pth`` into it)."""
        if not torch.cuda.is_available():
            raise RuntimeError("RewardScorer needs a GPU: the scoring stage has no CPU fallback")
        self.device = torch.device(device)
        self.input_size = input_size
        self.w = []
        for li, (n, k) in zip(_LINEARS, _SHAPES):
            k = input_size if k is None else k
            w = torch.as_tensor(aesthetic_state_dict[f"layers.{li}.weight"], dtype=F32)
            b = torch.as_tensor(aesthetic_state_dict[f"layers.{li}.bias"], dtype=F32)
            if tuple(w.shape) != (n, k) or tuple(b.shape) != (n,):
                raise ValueError(f"layers.{li}: weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected ({n}, {k}) / ({n},)")
            self.w.append((w.to(self.device).contiguous(), b.to(self.device).contiguous()))

    @torch.no_grad()
    def score(self, txt_features: torch.Tensor, img_pred_features: torch.Tensor, img_gt_features: torch.Tensor,
              miou: Optional[torch.Tensor] = None, laysim: Optional[torch.Tensor] = None) -> dict:
        """features: fp32 [B, D] CLIP embeddings (``get_text_features`` / ``get_image_features``, unnormalised).
        Returns dict(sims_ti, sims_ii, clip_reward, aes_reward, reward) of fp32 [B] device tensors; ``reward`` includes
        10 * miou + 10 * laysim when those (CPU-side layout terms, policy.py:126-133) are given."""
        f = lambda t: torch.as_tensor(t, dtype=F32).to(self.device).contiguous()
        t, p, g = f(txt_features), f(img_pred_features), f(img_gt_features)
        if not (t.shape == p.shape == g.shape) or t.dim() != 2 or t.shape[1] != self.input_size:
            raise ValueError(f"features must all be [B, {self.input_size}]")
        B = t.shape[0]
        out = torch.empty(4, B, dtype=F32, device=self.device)
        a = RewardArgs()
        a.txt, a.img_pred, a.img_gt, a.B, a.D = t.data_ptr(), p.data_ptr(), g.data_ptr(), B, self.input_size
        for i, (w, b) in enumerate(self.w, start=1):
            setattr(a, f"w{i}", w.data_ptr())
            setattr(a, f"b{i}", b.data_ptr())
        a.sims_ti, a.sims_ii, a.aesthetic, a.partial_reward = (out[i].data_ptr() for i in range(4))
        with torch.cuda.device(self.device):
            check(_lib.lib().gl_reward_score(C.byref(a), torch.cuda.current_stream(self.device).cuda_stream), "gl_reward_score")
        reward = out[3]
        if miou is not None:
            reward = reward + f(miou) * 10
        if laysim is not None:
            reward = reward + f(laysim) * 10
        return dict(sims_ti=out[0], sims_ii=out[1], clip_reward=out[0] + out[1], aes_reward=out[2], reward=reward)


class RewardModel:
    """GPU part of ``Reward_Model.forward`` (models/policy.py:106-124,135): CLIP text / image features -> cosine
    similarities + aesthetic score -> reward.  ``clip_state_dict`` = ``transformers.CLIPModel.state_dict()`` of the model
    policy.py:40 loads, ``aesthetic_state_dict`` = the AestheticMLP checkpoint (policy.py:44-46)."""

    def __init__(self, clip_state_dict, aesthetic_state_dict, device="cuda:0", vision_heads: int = 16, text_heads: int = 12, image_size: int = 224):
        from .clip import ClipTowers
        self.towers = ClipTowers(clip_state_dict, vision_heads, text_heads, device)
        self.scorer = RewardScorer(aesthetic_state_dict, device, input_size=int(self.towers.vproj.shape[0]))
        self.device = self.towers.device
        from .preprocess import ClipImagePreprocessor
        # self.processor(images=...) of policy.py:109,111, on the GPU (image_size = the checkpoint's vision_config.image_size)
        self.preprocess = ClipImagePreprocessor(size=image_size, crop_size=image_size, device=self.device)

    @torch.no_grad()
    def forward(self, input_ids, pixel_values_pred, pixel_values_gt, attention_mask=None, miou=None, laysim=None) -> dict:
        """``input_ids`` [B, T] (tokenizer output), ``pixel_values_*`` [B, 3, S, S] (processor output); returns the dict of
        RewardScorer.score plus the three feature tensors."""
        txt = self.towers.get_text_features(input_ids, attention_mask)
        pp_, pg_ = torch.as_tensor(pixel_values_pred), torch.as_tensor(pixel_values_gt)
        if pp_.shape[1:] == pg_.shape[1:]:
            # one pass of the vision tower over predictions + ground truth (rows are independent; twice the rows per GEMM)
            both = self.towers.get_image_features(torch.cat([pp_.to(self.device), pg_.to(self.device)], 0))
            pred, gt = both[:pp_.shape[0]], both[pp_.shape[0]:]
        else:
            pred = self.towers.get_image_features(pp_)
            gt = self.towers.get_image_features(pg_)
        out = self.scorer.score(txt, pred, gt, miou, laysim)
        out.update(txt_features=txt, img_pred_features=pred, img_gt_features=gt)
        return out

    @torch.no_grad()
    def forward_images(self, input_ids, images_pred, images_gt, attention_mask=None, miou=None, laysim=None,
                       pred_is_pixel_values: bool = False, gt_is_pixel_values: bool = False) -> dict:
        """``forward`` from IMAGES, as the reference's takes them (policy.py:106-111): ``images_pred`` is the VAE decoder's fp32
        output [B, 3, H, W] in [-1, 1] still on the GPU (converted to the uint8 pixels of interface.py:543-547 there), a uint8
        [B, H, W, 3] GPU tensor, or a list of PIL images; ``images_gt`` a list of PIL images / uint8 arrays of any sizes.
        The CLIP feature extractor's resize / crop / normalise runs on the GPU (preprocess.py), bit-identical to the PIL path.
        Ready ``pixel_values`` (processor output) are passed through ONLY when the caller says so with ``*_is_pixel_values``:
        an fp32 [B, 3, S, S] tensor is otherwise always taken as decoded images (a VAE output of the crop size is not
        pixel_values)."""
        def px(im, ready):
            if ready:
                if not (torch.is_tensor(im) and im.dtype == torch.float32 and im.dim() == 4 and im.shape[1] == 3):
                    raise TypeError("pixel_values must be an fp32 [B, 3, S, S] tensor")
                return im
            if torch.is_tensor(im) and im.dtype == torch.uint8:
                return self.preprocess(im.to(self.device))
            if torch.is_tensor(im):
                return self.preprocess.from_decoded(im)
            return self.preprocess.from_pil(im)
        return self.forward(input_ids, px(images_pred, pred_is_pixel_values), px(images_gt, gt_is_pixel_values), attention_mask, miou, laysim)

    # ------------------------------------------------------------------ the layout half (policy.py:53-102,126-135)
    @torch.no_grad()
    def emb_labels(self, labels: Sequence[str], input_ids, attention_mask=None) -> torch.Tensor:
        """``Reward.emb_labels`` (policy.py:54-72): the closed label set, its index and its L2-normalised text features [L, D] (kept on
        the device as ``labels_emb``).  ``input_ids`` / ``attention_mask``: the caller's tokenizer output for ``labels`` (padding=True)."""
        self.labels = list(labels)
        self.label2index = {l: i for i, l in enumerate(self.labels)}
        emb = self.towers.get_text_features(input_ids, attention_mask)
        if emb.shape[0] != len(self.labels):
            raise ValueError(f"{len(self.labels)} labels but {emb.shape[0]} token rows")
        self.labels_emb = torch.nn.functional.normalize(emb.float(), dim=-1)
        return self.labels_emb

    def _need_labels(self):
        if getattr(self, "labels_emb", None) is None:
            raise RuntimeError("call emb_labels(labels, input_ids) first: the label table is not set")

    @torch.no_grad()
    def nn_close_set(self, layouts: Sequence, tokenize: Callable) -> list:
        """``Reward.nn_close_set`` (policy.py:84-102): every label outside the closed set becomes the set's nearest label by CLIP text
        similarity.  ``tokenize``: list of strings -> (input_ids, attention_mask).  ONE text-tower run over the distinct unknown labels of
        the whole batch (the reference: one forward per occurrence); normalise, the product with the label table and the argmax run on the
        device, one [U] index vector comes back."""
        self._need_labels()
        unknown = []
        for _, labels in layouts:
            for l in labels:
                if l not in self.label2index and l not in unknown:
                    unknown.append(l)
        nearest = {}
        if unknown:
            ids, mask = tokenize(list(unknown))
            emb = torch.nn.functional.normalize(self.towers.get_text_features(ids, mask).float(), dim=-1)
            idx = (emb @ self.labels_emb.t()).argmax(dim=-1).tolist()
            nearest = {l: self.labels[i] for l, i in zip(unknown, idx)}
        return [(boxes, [l if l in self.label2index else nearest[l] for l in labels]) for boxes, labels in layouts]

    def label_to_id(self, layouts: Sequence) -> list:
        """``Reward.label_to_id`` (policy.py:74-82): (boxes, label names) -> (np.array(boxes), np.array(ids)); KeyError for a name outside the set"""
        self._need_labels()
        return [(np.array(boxes), np.array([self.label2index[l] for l in labels])) for boxes, labels in layouts]

    @torch.no_grad()
    def forward_layouts(self, input_ids, images_pred, images_gt, layout_pred, layout_gt, tokenize: Callable, attention_mask=None,
                        pred_is_pixel_values: bool = False, gt_is_pixel_values: bool = False) -> dict:
        """The whole of ``Reward.forward`` (policy.py:106-137) from images and layouts of (boxes, label NAMES): the predicted layouts go
        through ``nn_close_set``, both through ``label_to_id``, the two layout terms come from ``layout_terms`` and enter ``forward_images``.
        Returns its dict plus ``miou`` and ``laysim`` (float64 [B] device tensors); ``reward`` follows ``RewardScorer.score``'s dtype rule
        (fp32)."""
        pred_id = self.label_to_id(self.nn_close_set(layout_pred, tokenize))
        gt_id = self.label_to_id(layout_gt)
        terms = layout_terms(gt_id, pred_id, self.device)
        out = self.forward_images(input_ids, images_pred, images_gt, attention_mask, terms["miou"], terms["laysim"],
                                  pred_is_pixel_values, gt_is_pixel_values)
        out.update(miou=terms["miou"], laysim=terms["laysim"])
        return out

    __call__ = forward
