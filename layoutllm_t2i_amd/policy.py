"""In-context example selection of LayoutLLM-T2I on the MI355X: the policy layer's scores, the ranking and the rollout's
probabilities in one stream-ordered library call (``gl_policy_select``, csrc/policy.hip).

The reference projects the CLIP text features of the prompts and of the whole candidate pool through one trained ``nn.Linear``
(models/policy.py:11-33), multiplies the two (train_rl.py:167-170, txt2img.py:472-474) and then either ranks the row on the host
(txt2img.py:429-431) or samples from ``softmax(scores / policy_temperature)`` (train_rl.py:172, :38-48).  Here

* ``PolicyNetwork`` holds the layer (``load_state_dict`` takes ``policy_model.linear.state_dict()``, train_rl.py:219 / txt2img.py:551)
  and returns ``scores`` / ``probabilities`` / ``select`` as device tensors;
* ``CandidatePool`` keeps the candidate records with their CLIP text features, embedded once on the HIP text tower;
* ``sample_examples`` is the host part of the rollout, from numpy's stream like the reference.

The log-probability sum, the policy gradient and the optimiser step (train_rl.py:85-95, :182-184) are ``policy_train.PolicyTrainer``, which
updates this network's layer in place; the trainer's loop is ``train_rl``.
No fallback: without a GPU / the library the scoring raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import PolicyArgs

F32 = torch.float32
MAX_PROMPTS = 64         # GL_POLICY_MAX_PROMPTS: more prompts are processed in chunks
MAX_DIM = 1024           # GL_POLICY_MAX_DIM
MAX_SHOTS = 32           # GL_POLICY_MAX_SHOTS
MIN_TOKEN_ROWS = 1536    # CandidatePool.from_captions: token rows per text-tower call from which a row's feature is batch-invariant (with margin)


class PolicyNetwork:
    def __init__(self, in_dim: int = 768, embedding_size: int = 128, add_linear: bool = True, device="cuda:0"):
        """``add_linear=False``: no layer, the score is the plain inner product of the features (models/policy.py:23-24)."""
        self.in_dim, self.add_linear = int(in_dim), bool(add_linear)
        self.embedding_size = int(embedding_size) if add_linear else int(in_dim)
        if self.in_dim % 4 or not 4 <= self.in_dim <= MAX_DIM:
            raise ValueError(f"in_dim = {in_dim}: the kernel takes a multiple of 4 up to {MAX_DIM}")
        if not 1 <= self.embedding_size <= MAX_DIM:
            raise ValueError(f"embedding_size = {embedding_size}: the kernel takes 1 .. {MAX_DIM}")
        self.device = torch.device(device)
        self.weight = self.bias = None

    def load_state_dict(self, state_dict: Mapping[str, object]) -> "PolicyNetwork":
        """``policy_model.linear.state_dict()``: ``weight`` [embedding_size, in_dim] and ``bias`` [embedding_size]"""
        if not self.add_linear:
            raise ValueError("add_linear=False: this policy has no layer to load")
        missing = [k for k in ("weight", "bias") if k not in state_dict]
        if missing:
            raise ValueError(f"state dict without {missing}: expected the keys of policy_model.linear.state_dict()")
        w, b = (torch.as_tensor(state_dict[k]).detach() for k in ("weight", "bias"))
        if tuple(w.shape) != (self.embedding_size, self.in_dim) or tuple(b.shape) != (self.embedding_size,):
            raise ValueError(f"weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected ({self.embedding_size}, {self.in_dim}) / ({self.embedding_size},)")
        self.weight, self.bias = w.to(self.device, F32).contiguous(), b.to(self.device, F32).contiguous()
        return self

    # ------------------------------------------------------------------ the library call
    def _operand(self, t, name: str) -> torch.Tensor:
        t = torch.as_tensor(t)
        if t.dim() != 2 or t.shape[1] != self.in_dim or t.shape[0] < 1:
            raise ValueError(f"{name} {tuple(t.shape)}, expected [n >= 1, {self.in_dim}]")
        t = t.detach().to(self.device, F32).contiguous()
        return t.clone() if t.data_ptr() % 16 else t

    def _call(self, prompt: torch.Tensor, cand: torch.Tensor, k: int, temperature: Optional[float]):
        """one gl_policy_select over at most 64 prompts -> (scores [P, N], topk int32 [P, k] or None, probs [P, N] or None)"""
        if self.device.type != "cuda":
            raise RuntimeError("the policy scoring runs on the GPU only (there is no CPU fallback)")
        if self.add_linear and self.weight is None:
            raise RuntimeError("load_state_dict first: the policy layer has no weights")
        P, N = int(prompt.shape[0]), int(cand.shape[0])
        lib = _lib.lib()
        nbytes = int(lib.gl_policy_scratch_bytes(P, N, self.in_dim, self.embedding_size, k, int(not self.add_linear), int(temperature is not None)))
        if nbytes < 0:
            raise ValueError(f"gl_policy_scratch_bytes refused P = {P}, N = {N}, k = {k}")
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        scores = torch.empty(P, N, dtype=F32, device=self.device)
        topk = torch.empty(P, k, dtype=torch.int32, device=self.device) if k > 0 else None
        probs = torch.empty(P, N, dtype=F32, device=self.device) if temperature is not None else None
        a = PolicyArgs()
        a.prompt, a.cand = prompt.data_ptr(), cand.data_ptr()
        a.W, a.bias = (self.weight.data_ptr(), self.bias.data_ptr()) if self.add_linear else (None, None)
        a.P, a.N, a.D, a.E, a.k = P, N, self.in_dim, self.embedding_size, k
        a.temperature = float(temperature) if temperature is not None else 1.0
        a.scores = scores.data_ptr()
        a.topk = topk.data_ptr() if topk is not None else None
        a.probs = probs.data_ptr() if probs is not None else None
        a.scratch, a.scratch_bytes = scratch.data_ptr(), nbytes
        with torch.cuda.device(self.device):
            rc = lib.gl_policy_select(C.byref(a), torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise _lib.HipLibraryError(f"gl_policy_select failed with code {rc}: {_lib.last_error(None)}")
        return scores, topk, probs

    def _run(self, emb_prompt, emb_cand, k: int = 0, temperature: Optional[float] = None):
        prompt, cand = self._operand(emb_prompt, "emb_prompt"), self._operand(emb_cand, "emb_cand")
        parts = [self._call(prompt[i:i + MAX_PROMPTS], cand, k, temperature) for i in range(0, prompt.shape[0], MAX_PROMPTS)]
        if len(parts) == 1:
            return parts[0]
        return tuple(None if col[0] is None else torch.cat(col, 0) for col in zip(*parts))

    @torch.no_grad()
    def scores(self, emb_prompt, emb_cand) -> torch.Tensor:
        """``torch.mm(policy_model(emb_prompt), policy_model(emb_cand).t())`` (txt2img.py:472-474): fp32 [P, N] on the device"""
        return self._run(emb_prompt, emb_cand)[0]

    @torch.no_grad()
    def probabilities(self, emb_prompt, emb_cand, temperature: float = 1.0) -> torch.Tensor:
        """``F.softmax(scores / policy_temperature, dim=1)`` (train_rl.py:172): fp32 [P, N] on the device"""
        if not temperature > 0:
            raise ValueError(f"temperature = {temperature}: must be > 0")
        return self._run(emb_prompt, emb_cand, 0, temperature)[2]

    @torch.no_grad()
    def select(self, emb_prompt, emb_cand, shot_number: int) -> torch.Tensor:
        """The ``cids`` of txt2img.py:429-431 for every prompt: the ``shot_number`` best candidates, equal scores by the lower index,
        REVERSED so that the most relevant example comes last; int64 [P, min(shot_number, N)] on the device."""
        k = int(shot_number)
        if not 0 <= k <= MAX_SHOTS:
            raise ValueError(f"shot_number = {shot_number}: the kernel ranks 0 .. {MAX_SHOTS} examples")
        if k == 0:
            return torch.empty(int(self._operand(emb_prompt, "emb_prompt").shape[0]), 0, dtype=torch.int64, device=self.device)
        topk = self._run(emb_prompt, emb_cand, k)[1]
        return topk[:, :min(k, int(torch.as_tensor(emb_cand).shape[0]))].flip(1).to(torch.int64)


class CandidatePool:
    """The candidate records (dicts with ``captions``, ``label``, ``bbox``: ``raw['data']`` of the reference's candidate JSON,
    txt2img.py:466-468) with the CLIP text features of their captions, fp32 [N, D], kept on the device.  ``towers``: the text tower the
    pool was embedded with (``from_captions`` sets it); ``txt2img.generate`` embeds the prompt with the same one."""

    def __init__(self, examples: Sequence[Mapping], features: torch.Tensor, towers=None):
        self.examples = list(examples)
        self.features = torch.as_tensor(features)
        if not self.examples:
            raise ValueError("an empty candidate pool")
        if self.features.dim() != 2 or self.features.shape[0] != len(self.examples):
            raise ValueError(f"{len(self.examples)} examples but features {tuple(self.features.shape)}")
        self.towers = towers

    def __len__(self):
        return len(self.examples)

    @classmethod
    @torch.no_grad()
    def from_captions(cls, examples: Sequence[Mapping], towers_or_clip, tokenize: Callable, batch: int = 256) -> "CandidatePool":
        """Embeds ``ex['captions']`` of every example (txt2img.py:468-469).  ``towers_or_clip``: ``clip.ClipTowers`` (the HIP text tower) or
        anything with its ``get_text_features(input_ids, attention_mask)``; ``tokenize``: list of strings -> (input_ids, attention_mask),
        the caller's tokenizer with ``padding=True``.

        The features are those of ONE ``get_text_features`` call over the whole pool, bit for bit, whatever ``batch`` is.  The HIP
        tower's GEMM launcher picks its kernel from the tile count, so a row's feature depends on the number of token rows in the call
        until there are enough of them (measured on an MI355X: no dependence from 1 232 token rows on, up to the 39 424 tried, at 16, 32
        and 77 tokens per caption).  So: the captions are tokenised once (every call has the pool's padded length); a pool that fits one
        call is one call; otherwise every call carries the same number of rows, ``batch`` raised to ``MIN_TOKEN_ROWS`` token rows if it
        is smaller, and the last call is filled up with copies of the pool's first row (dropped again)."""
        if batch < 1:
            raise ValueError(f"batch = {batch}")
        examples = list(examples)
        if not examples:
            raise ValueError("an empty candidate pool")
        ids, mask = tokenize([ex["captions"] for ex in examples])
        N, T = int(ids.shape[0]), int(ids.shape[1])
        rows = max(int(batch), -(-MIN_TOKEN_ROWS // T))
        if N <= rows:
            return cls(examples, towers_or_clip.get_text_features(input_ids=ids, attention_mask=mask).clone(), towers_or_clip)
        feats = None
        for i in range(0, N, rows):
            bi, bm = ids[i:i + rows], None if mask is None else mask[i:i + rows]
            n = int(bi.shape[0])
            if n < rows:
                bi = torch.cat([bi, ids[:1].expand(rows - n, T)], 0)
                bm = None if bm is None else torch.cat([bm, mask[:1].expand(rows - n, T)], 0)
            f = towers_or_clip.get_text_features(input_ids=bi, attention_mask=bm)
            if feats is None:
                feats = torch.empty(N, f.shape[1], dtype=F32, device=f.device)
            feats[i:i + n] = f[:n]                       # (a copy: the tower's captured graph returns its own output buffer)
        return cls(examples, feats, towers_or_clip)


@torch.no_grad()
def embed_texts(towers_or_clip, tokenize: Callable, texts: Sequence[str]) -> torch.Tensor:
    """CLIP text features [n, D] of ``texts``, a fresh tensor (``extract_text_feat``, txt2img.py:454-457)"""
    ids, mask = tokenize(list(texts))
    return towers_or_clip.get_text_features(input_ids=ids, attention_mask=mask).clone()


def sample_examples(prob_row, shot_number: int, rng=np.random) -> np.ndarray:
    """The host part of the rollout (train_rl.py:38-48) for one row of ``probabilities``: NaN -> 1e-6, renormalise, draw
    ``shot_number`` distinct candidates with these probabilities from numpy's stream (``rng``: ``np.random`` or a RandomState /
    Generator), reversed like the ranked selection.  The row keeps its dtype (fp32 from the device), as in the reference."""
    p = prob_row.detach().cpu().numpy() if torch.is_tensor(prob_row) else np.array(prob_row)
    p = np.nan_to_num(p, nan=0.000001)
    p /= p.sum()
    cids = rng.choice(range(len(p)), shot_number, p=p, replace=False)
    return cids[::-1]
