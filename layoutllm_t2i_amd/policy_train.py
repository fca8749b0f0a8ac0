"""Training LayoutLLM-T2I's example-selection policy on the MI355X: the REINFORCE loss of one rollout batch with its gradient to the
policy layer (``gl_policy_grad``) and the Adam step on that layer (``gl_policy_adam_step``), both in csrc/policy_train.hip.

The reference builds the loss from the softmax of the scores and ``torch.log`` of the sampled entries (train_rl.py:167-172, :85-95), lets
autograd differentiate it and updates the layer with ``torch.optim.Adam`` under a ``StepLR`` (train_rl.py:119-120, :182-184, :250).
``PolicyTrainer`` does the same on the weights a ``policy.PolicyNetwork`` holds, in place: there is no second copy of the layer, and the
next ``scores`` / ``select`` / ``probabilities`` call of that network sees the updated one.

``state_dict`` / ``load_state_dict`` speak the layout of the reference's ``state_{epoch}.pt`` (train_rl.py:221): ``{'optimizer':
Adam.state_dict(), 'lr_scheduler': StepLR.state_dict()}``, parameter 0 the weight, parameter 1 the bias, so a file written by either side
resumes on the other.  The layer itself is saved as ``policy_model.linear.state_dict()`` is: ``weights()``.

No fallback: without a GPU / the library ``loss_and_grad`` and ``step`` raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import numpy as np
import torch

from . import _lib
from ._lib import PolicyAdamArgs, PolicyGradArgs
from .policy import MAX_PROMPTS, MAX_SHOTS, PolicyNetwork

F32, F64 = torch.float32, torch.float64
MAX_TRAIN_CANDS = 4096      # GL_POLICY_TRAIN_MAX_CANDS


class PolicyTrainer:
    def __init__(self, policy: PolicyNetwork, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, lr_step_size: int = 20,
                 lr_gamma: float = 0.5):
        """``policy``: a ``PolicyNetwork`` with its layer loaded; the trainer updates ``policy.weight`` / ``policy.bias`` in place.
        ``lr`` / ``betas`` / ``eps``: ``torch.optim.Adam``'s (weight_decay 0, no amsgrad); ``lr_step_size`` / ``lr_gamma``: ``StepLR``'s."""
        if not policy.add_linear:
            raise ValueError("add_linear=False: the identity policy has no layer to train")
        if policy.weight is None:
            raise ValueError("load_state_dict first: the policy layer has no weights to train")
        if not lr >= 0 or not eps >= 0 or not all(0 <= b < 1 for b in betas) or len(betas) != 2:
            raise ValueError(f"lr = {lr}, betas = {betas}, eps = {eps}: need lr >= 0, eps >= 0, betas in [0, 1)")
        if int(lr_step_size) < 1:
            raise ValueError(f"lr_step_size = {lr_step_size}: must be >= 1")
        self.policy = policy
        self.base_lr = self.lr = float(lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.lr_step_size, self.lr_gamma = int(lr_step_size), float(lr_gamma)
        self.steps = 0          # Adam's step count
        self.epochs = 0         # StepLR's last_epoch
        w, b = policy.weight, policy.bias
        self.exp_avg = [torch.zeros_like(w), torch.zeros_like(b)]
        self.exp_avg_sq = [torch.zeros_like(w), torch.zeros_like(b)]

    # ------------------------------------------------------------------ the library calls
    def _inputs(self, emb_prompt, emb_cand, sel, reward, temperature):
        """shape and range checks, before a device is needed -> the host-side operands"""
        net = self.policy
        prompt, cand = torch.as_tensor(emb_prompt), torch.as_tensor(emb_cand)
        for t, name in ((prompt, "emb_prompt"), (cand, "emb_cand")):
            if t.dim() != 2 or t.shape[1] != net.in_dim or t.shape[0] < 1:
                raise ValueError(f"{name} {tuple(t.shape)}, expected [n >= 1, {net.in_dim}]")
        P, N = int(prompt.shape[0]), int(cand.shape[0])
        if P > MAX_PROMPTS:
            raise ValueError(f"{P} prompts: one update takes at most {MAX_PROMPTS} (GL_POLICY_MAX_PROMPTS)")
        if N > MAX_TRAIN_CANDS:
            raise ValueError(f"{N} candidates: the trainer takes at most {MAX_TRAIN_CANDS} (GL_POLICY_TRAIN_MAX_CANDS)")
        sel = torch.as_tensor(np.asarray(sel) if not torch.is_tensor(sel) else sel)
        if sel.dim() != 2 or sel.shape[0] != P or not 1 <= sel.shape[1] <= MAX_SHOTS or sel.is_floating_point():
            raise ValueError(f"sel {tuple(sel.shape)} {sel.dtype}: expected integers [P = {P}, k in 1 .. {MAX_SHOTS}]")
        reward = torch.as_tensor(reward)
        if tuple(reward.shape) != (P,) or not reward.is_floating_point():
            raise ValueError(f"reward {tuple(reward.shape)} {reward.dtype}: expected floats [P = {P}]")
        if not temperature > 0:
            raise ValueError(f"temperature = {temperature}: must be > 0")
        if net.device.type != "cuda":
            raise RuntimeError("the policy gradient runs on the GPU only (there is no CPU fallback)")
        return net._operand(prompt, "emb_prompt"), net._operand(cand, "emb_cand"), sel, reward

    def loss_and_grad(self, emb_prompt, emb_cand, sel, reward, temperature: float = 1.0) -> dict:
        """The loss of train_rl.py:95 and its gradient to the layer.  ``sel``: int [P, k], the sampled pool indices of every prompt (an entry
        outside [0, N) is skipped; a repeated one counts as often as it occurs); ``reward``: [P] of any float dtype.  Returns
        ``dict(loss, log_prob, grad_weight, grad_bias)``: device tensors, ``loss`` (0-dim) and ``log_prob`` [P] in double; nothing is
        synchronised and the layer is not touched."""
        net = self.policy
        prompt, cand, sel, reward = self._inputs(emb_prompt, emb_cand, sel, reward, temperature)
        dev = net.device
        P, N, k = int(prompt.shape[0]), int(cand.shape[0]), int(sel.shape[1])
        sel = sel.detach().to(dev, torch.int32).contiguous()
        reward = reward.detach().to(dev, F64).contiguous()
        lib = _lib.lib()
        nbytes = int(lib.gl_policy_grad_scratch_bytes(P, N, net.in_dim, net.embedding_size, k))
        if nbytes < 0:
            raise ValueError(f"gl_policy_grad_scratch_bytes refused P = {P}, N = {N}, k = {k}")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty(1, dtype=F64, device=dev)
        logp = torch.empty(P, dtype=F64, device=dev)
        gw, gb = torch.empty_like(net.weight), torch.empty_like(net.bias)
        a = PolicyGradArgs()
        a.prompt, a.cand, a.W, a.bias = prompt.data_ptr(), cand.data_ptr(), net.weight.data_ptr(), net.bias.data_ptr()
        a.sel, a.reward = sel.data_ptr(), reward.data_ptr()
        a.P, a.N, a.D, a.E, a.k, a.temperature = P, N, net.in_dim, net.embedding_size, k, float(temperature)
        a.loss, a.logp, a.grad_W, a.grad_b = loss.data_ptr(), logp.data_ptr(), gw.data_ptr(), gb.data_ptr()
        a.scratch, a.scratch_bytes = scratch.data_ptr(), nbytes
        with torch.cuda.device(dev):
            rc = lib.gl_policy_grad(C.byref(a), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise _lib.HipLibraryError(f"gl_policy_grad failed with code {rc}: {_lib.last_error(None)}")
        return dict(loss=loss[0], log_prob=logp, grad_weight=gw, grad_bias=gb)

    def step(self, emb_prompt, emb_cand, sel, reward, temperature: float = 1.0) -> dict:
        """``loss_and_grad``, then one Adam step on ``policy.weight`` / ``policy.bias`` in place (train_rl.py:182-184).  Returns the same
        dict: the loss and the gradient at the weights BEFORE the step."""
        out = self.loss_and_grad(emb_prompt, emb_cand, sel, reward, temperature)
        net = self.policy
        self.steps += 1
        a = PolicyAdamArgs()
        a.W, a.bias = net.weight.data_ptr(), net.bias.data_ptr()
        a.grad_W, a.grad_b = out["grad_weight"].data_ptr(), out["grad_bias"].data_ptr()
        a.exp_avg_W, a.exp_avg_sq_W = self.exp_avg[0].data_ptr(), self.exp_avg_sq[0].data_ptr()
        a.exp_avg_b, a.exp_avg_sq_b = self.exp_avg[1].data_ptr(), self.exp_avg_sq[1].data_ptr()
        a.D, a.E, a.step = net.in_dim, net.embedding_size, self.steps
        a.lr, a.beta1, a.beta2, a.eps = self.lr, self.betas[0], self.betas[1], self.eps
        with torch.cuda.device(net.device):
            rc = _lib.lib().gl_policy_adam_step(C.byref(a), torch.cuda.current_stream(net.device).cuda_stream)
        if rc != 0:
            self.steps -= 1
            raise _lib.HipLibraryError(f"gl_policy_adam_step failed with code {rc}: {_lib.last_error(None)}")
        return out

    # ------------------------------------------------------------------ the schedule
    def epoch_end(self) -> float:
        """``StepLR.step()`` (train_rl.py:250): lr = base_lr * gamma ** (epochs // step_size)"""
        self.epochs += 1
        self.lr = self.base_lr * self.lr_gamma ** (self.epochs // self.lr_step_size)
        return self.lr

    def set_lr(self, lr: float) -> None:
        """The reference's "use new learning rate" after a resume (train_rl.py:129-130): Adam's moments and step count stay, the schedule
        starts again from ``lr`` (the reference builds a fresh StepLR and never loads the saved one)."""
        if not lr >= 0:
            raise ValueError(f"lr = {lr}: must be >= 0")
        self.base_lr = self.lr = float(lr)
        self.epochs = 0

    # ------------------------------------------------------------------ checkpoints
    def weights(self) -> dict:
        """``policy_model.linear.state_dict()`` (train_rl.py:219): CPU copies under ``weight`` and ``bias``"""
        return {"weight": self.policy.weight.detach().cpu().clone(), "bias": self.policy.bias.detach().cpu().clone()}

    def _templates(self):
        """state dicts of a real Adam / StepLR with this trainer's settings: whatever keys this torch version writes"""
        params = [torch.nn.Parameter(torch.zeros(0)), torch.nn.Parameter(torch.zeros(0))]
        opt = torch.optim.Adam(params, lr=self.base_lr, betas=self.betas, eps=self.eps)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=self.lr_step_size, gamma=self.lr_gamma)
        return opt.state_dict(), sched.state_dict()

    def state_dict(self) -> dict:
        """``{'optimizer': ..., 'lr_scheduler': ...}`` as train_rl.py:221 saves them; tensors on the CPU"""
        opt, sched = self._templates()
        group = opt["param_groups"][0]
        group["lr"], group["initial_lr"], group["params"] = self.lr, self.base_lr, [0, 1]
        opt["state"] = {} if self.steps == 0 else {
            i: {"step": torch.tensor(float(self.steps)), "exp_avg": self.exp_avg[i].detach().cpu().clone(),
                "exp_avg_sq": self.exp_avg_sq[i].detach().cpu().clone()} for i in (0, 1)}
        sched.update(step_size=self.lr_step_size, gamma=self.lr_gamma, base_lrs=[self.base_lr], last_epoch=self.epochs,
                     _step_count=self.epochs + 1, _last_lr=[self.lr])
        return {"optimizer": opt, "lr_scheduler": sched}

    def load_state_dict(self, d: Mapping) -> "PolicyTrainer":
        """The dict of ``state_dict`` or of the reference's ``state_{epoch}.pt``; ``lr_scheduler`` may be missing (the reference's resume
        loads the optimizer alone, train_rl.py:112)."""
        if "optimizer" not in d:
            raise ValueError("state dict without 'optimizer': expected the keys of the reference's state_{epoch}.pt")
        opt = d["optimizer"]
        groups = opt.get("param_groups", [])
        if len(groups) != 1 or list(groups[0].get("params", [])) != [0, 1]:
            raise ValueError("optimizer state: expected one parameter group over parameters [0, 1] (weight, bias)")
        g = groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("optimizer state with weight_decay / amsgrad / maximize: the step kernel is the reference's plain Adam")
        state = opt.get("state", {})
        w, b = self.policy.weight, self.policy.bias
        if len(state) == 0:
            steps, avg, sq = 0, [torch.zeros_like(w), torch.zeros_like(b)], [torch.zeros_like(w), torch.zeros_like(b)]
        else:
            if sorted(state) != [0, 1]:
                raise ValueError(f"optimizer state for parameters {sorted(state)}, expected [0, 1]")
            counts = {int(state[i]["step"]) for i in (0, 1)}
            if len(counts) != 1:
                raise ValueError(f"optimizer state with different step counts {sorted(counts)} for weight and bias")
            steps = counts.pop()
            avg, sq = [], []
            for i, p in ((0, w), (1, b)):
                for key, dst in (("exp_avg", avg), ("exp_avg_sq", sq)):
                    t = torch.as_tensor(state[i][key]).detach()
                    if t.shape != p.shape:
                        raise ValueError(f"optimizer state {key} of parameter {i} {tuple(t.shape)}, expected {tuple(p.shape)}")
                    dst.append(t.to(p.device, F32).contiguous().clone())
        self.steps, self.exp_avg, self.exp_avg_sq = steps, avg, sq
        self.lr = float(g["lr"])
        self.betas, self.eps = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        self.base_lr = float(g.get("initial_lr", self.lr))
        sched = d.get("lr_scheduler")
        if sched is not None:
            self.lr_step_size, self.lr_gamma = int(sched["step_size"]), float(sched["gamma"])
            self.base_lr, self.epochs = float(sched["base_lrs"][0]), int(sched["last_epoch"])
        return self
