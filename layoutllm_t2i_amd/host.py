"""Host-side (CPU, once per image) pieces of the denoising path: integer box rectangles for the
relation injection, the alpha (fuser-scale) schedule and the PLMS / DDIM / DPM-Solver++ schedule tables.

Everything here is tiny scalar/table work that the reference redoes inside its hot loop
(attention.py:321-346 with 4 ``.tolist()`` device syncs per call x 16 layers x 102 forwards;
plms.py:60 per sample() call); it is hoisted out of the loop, result-identically.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np


def box_rects(boxes: np.ndarray, masks: np.ndarray, h: int, w: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Pixel rectangles of RelationCrossAttention.forward (attention.py:321-346) for one resolution.

    boxes [B, n, 4] float32 (x0, y0, x1, y1 normalised), masks [B, n] float32.
    Returns (rects [B, n, 4] int32 = (top, bottom, left, right) *already normalised to the effective
    python-slice range*, nvalid [B] int32 = number of boxes used before the reference's ``break`` at
    the first padded or degenerate box, poison [B] int32 = 1 where a used box has an empty slice
    (right < left or bottom < top), for which the reference yields NaN over the whole sample).

    Arithmetic mirrors the reference exactly: float32 multiply by the python int, truncation toward
    zero (``.to(torch.int)``), x1/y1 clamped to w/h with torch.minimum, x0/y0 not clamped.
    """
    boxes = np.asarray(boxes, dtype=np.float32)
    masks = np.asarray(masks, dtype=np.float32)
    B, n, _ = boxes.shape
    count = masks.sum(axis=-1)
    x0 = (boxes[:, :, 0] * w).astype(np.int32)
    y0 = (boxes[:, :, 1] * h).astype(np.int32)
    x1 = np.minimum(boxes[:, :, 2] * w, np.float32(w)).astype(np.int32)
    y1 = np.minimum(boxes[:, :, 3] * h, np.float32(h)).astype(np.int32)
    rects = np.zeros((B, n, 4), np.int32)
    nvalid = np.zeros((B,), np.int32)
    poison = np.zeros((B,), np.int32)
    for k in range(B):
        for i in range(n):
            left, right, top, bottom = int(x0[k, i]), int(x1[k, i]), int(y0[k, i]), int(y1[k, i])
            if i < count[k] and left != right and top != bottom:
                t, b, _ = slice(top, bottom).indices(h)     # python slice semantics incl. negatives
                l, r, _ = slice(left, right).indices(w)
                b, r = max(b, t), max(r, l)
                rects[k, i] = (t, b, l, r)
                if (b - t) * (r - l) == 0:
                    poison[k] = 1
                nvalid[k] = i + 1
            else:
                break
    return rects, nvalid, poison


def alpha_generator(length: int, type=None) -> List[float]:
    """Fuser scale per sampling step (interface.py:41-75): [1]*n0 + linear decay + [0]*n2."""
    if type is None:
        type = [1, 0, 0]
    assert len(type) == 3
    assert type[0] + type[1] + type[2] == 1
    n0 = int(type[0] * length)
    n1 = int(type[1] * length)
    n2 = length - n0 - n1
    decay = list(np.arange(start=0, stop=1, step=1 / n1)[::-1]) if n1 != 0 else []
    alphas = [1] * n0 + decay + [0] * n2
    assert len(alphas) == length
    return alphas


def alphas_cumprod(timesteps: int = 1000, linear_start: float = 0.00085, linear_end: float = 0.012) -> np.ndarray:
    """DDPM.register_schedule for the 'linear' schedule (util.py:31-34, ddpm.py:19-35): float64 betas,
    cumprod, stored as float32."""
    betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas, axis=0).astype(np.float32)


def make_schedule(S: int, acp: np.ndarray) -> Dict[str, np.ndarray]:
    """PLMSSampler.make_schedule with eta = 0 (plms.py:25-56; util.py:55-83)."""
    T = acp.shape[0]
    c = T // S
    ts = np.asarray(list(range(0, T, c))) + 1
    a = acp[ts].astype(np.float32)
    a_prev = np.asarray([acp[0]] + acp[ts[:-1]].tolist(), dtype=np.float64)
    return dict(ddim_timesteps=ts, ddim_alphas=a, ddim_alphas_prev=a_prev,
                ddim_sqrt_one_minus_alphas=np.sqrt(np.float32(1.0) - a), ddim_sigmas=np.zeros_like(a_prev))


# Adams-Bashforth combinations of plms.py:144-159: (coefficients of [e_t, old[-1], old[-2], old[-3]], divisor)
PLMS_COEFS = {
    0: ((1.0, 1.0), 2.0),                       # (e_t + e_t_next) / 2   (second evaluation on step 0)
    1: ((3.0, -1.0), 2.0),
    2: ((23.0, -16.0, 5.0), 12.0),
    3: ((55.0, -59.0, 37.0, -9.0), 24.0),
}


def step_coefs(sched: Dict[str, np.ndarray], index: int) -> Tuple[float, float, float, float]:
    """float32 scalars of get_x_prev_and_pred_x0 (plms.py:126-140) with sigma = 0:
    (sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev))."""
    a_t = np.float32(sched["ddim_alphas"][index])
    a_prev = np.float32(sched["ddim_alphas_prev"][index])
    s1m = np.float32(sched["ddim_sqrt_one_minus_alphas"][index])
    return (float(np.sqrt(a_t)), float(s1m), float(np.sqrt(a_prev)), float(np.sqrt(np.float32(1.0) - a_prev)))


DDIM_DISCRETIZE = ("uniform", "quad")


def check_ddim_eta(eta) -> float:
    """eta of the DDIM variance schedule: a finite number >= 0, else ValueError"""
    if isinstance(eta, bool) or not isinstance(eta, (int, float, np.integer, np.floating)) or not np.isfinite(eta) or eta < 0:
        raise ValueError(f"ddim_eta = {eta!r}: must be a finite number >= 0")
    return float(eta)


def make_ddim_schedule(S: int, acp: np.ndarray, discretize: str = "uniform", eta: float = 0.0) -> Dict[str, np.ndarray]:
    """DDIMSampler.make_schedule (ddim.py:27-50): make_ddim_timesteps (util.py:55-69) and make_ddim_sampling_parameters (util.py:72-83) in the
    reference's dtypes.  ``acp``: the float32 alphas_cumprod buffer.

    ddim_timesteps int64: 'uniform' = range(0, T, T // S) + 1 (S = 6 gives 7 of them), 'quad' = int(linspace(0, sqrt(0.8 T), S) ** 2) + 1
    (neighbours may coincide).  ddim_alphas float32 = acp[t]; ddim_alphas_prev float64 = [acp[0], acp[t[:-1]]];
    ddim_sqrt_one_minus_alphas float32 = sqrt(1 - alphas) in float32; ddim_sigmas float64 =
    eta * sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev)).  The reference divides a float64 numpy array by a float32 torch tensor there, which
    torch evaluates as ``reciprocal(1 - a) * (1 - a_prev)``: the difference and the reciprocal in float32, everything else in float64."""
    acp = np.asarray(acp, dtype=np.float32)
    T = acp.shape[0]
    if discretize == "uniform":
        ts = np.asarray(list(range(0, T, T // S)))
    elif discretize == "quad":
        ts = ((np.linspace(0, np.sqrt(T * .8), S)) ** 2).astype(int)
    else:
        raise ValueError(f"ddim_discretize = {discretize!r}: one of {DDIM_DISCRETIZE}")
    eta = check_ddim_eta(eta)
    ts = ts + 1
    a = acp[ts]
    a_prev = np.asarray([acp[0]] + acp[ts[:-1]].tolist(), dtype=np.float64)
    recip = (np.float32(1.0) / (np.float32(1.0) - a)).astype(np.float64)
    sigmas = eta * np.sqrt(recip * (1.0 - a_prev) * (1.0 - a.astype(np.float64) / a_prev))
    return dict(ddim_timesteps=ts, ddim_alphas=a, ddim_alphas_prev=a_prev, ddim_sqrt_one_minus_alphas=np.sqrt(np.float32(1.0) - a),
                ddim_sigmas=sigmas)


def ddim_step_coefs(sched: Dict[str, np.ndarray], index: int) -> Tuple[float, float, float, float, float]:
    """The float32 scalars of p_sample_ddim (ddim.py:121-133), each table entry rounded to float32 first (``torch.full``), the arithmetic in
    float32: (sqrt(a_t), sqrt(1 - a_t) from its table, sqrt(a_prev), sqrt(1 - a_prev - sigma_t ** 2), sigma_t)."""
    f = np.float32
    a_t, a_prev, sigma = f(sched["ddim_alphas"][index]), f(sched["ddim_alphas_prev"][index]), f(sched["ddim_sigmas"][index])
    s1m = f(sched["ddim_sqrt_one_minus_alphas"][index])
    dir_coef = np.sqrt(f(f(f(1.0) - a_prev) - f(sigma * sigma)))
    return (float(np.sqrt(a_t)), float(s1m), float(np.sqrt(a_prev)), float(dir_coef), float(sigma))


DPM_DISCRETIZE = ("logsnr", "quad", "uniform")
DPM_ORDERS = (2, 1)
DPM_LOWER_ORDER_FINAL = 15        # fewer evaluations than this: the last step is first order (the usual lower_order_final rule)


def _log_snr(a):
    """lambda = 1/2 log(a / (1 - a)) in float64: half the log signal-to-noise ratio at alphas_cumprod ``a``"""
    a = np.asarray(a, dtype=np.float64)
    return 0.5 * np.log(a / (1.0 - a))


def make_dpm_schedule(S: int, acp: np.ndarray, discretize: str = "logsnr") -> Dict[str, np.ndarray]:
    """Timesteps and nodes of the DPM-Solver++(2M) sampler (Lu et al., arXiv 2211.01095).  ``acp``: the float32 alphas_cumprod buffer.

    'logsnr': S targets ``linspace(lambda(1), lambda(T - 1), S)`` (float64); per target the t in [1, T - 1] with the nearest lambda; sorted
    ascending, repeats dropped (S = 10: [1, 6, 24, ..., 882, 999]; S = 1: [T - 1]).  'uniform' / 'quad': make_ddim_schedule's timesteps, repeats dropped (a
    step of width h = 0 would divide by zero in r).  Hence n = len(ddim_timesteps) may differ from S: <= S on 'logsnr' and 'quad', range()'s
    count on 'uniform' (S = 6 gives 7).

    The nodes as in DDIM: ddim_alphas float32 = acp[t], ddim_alphas_prev float64 = [acp[0], acp[t[:-1]]]; plus ``lambdas`` /
    ``lambdas_prev`` float64 = the half log-SNR of either, ``ddim_sqrt_one_minus_alphas`` float32, and ``ddim_sigmas`` = 0 (deterministic)."""
    acp = np.asarray(acp, dtype=np.float32)
    T = acp.shape[0]
    S = int(S)
    if S < 1:
        raise ValueError(f"steps = {S}: must be >= 1")
    if discretize == "logsnr":
        lam = _log_snr(acp[1:])                       # lam[k] = lambda(k + 1), decreasing in t
        targets = np.linspace(lam[0], lam[-1], S) if S > 1 else lam[-1:]      # one step: from t = T - 1, where the latent is noise
        ts = np.abs(lam[None, :] - targets[:, None]).argmin(axis=1) + 1
    elif discretize in ("uniform", "quad"):
        ts = make_ddim_schedule(S, acp, discretize)["ddim_timesteps"]
    else:
        raise ValueError(f"dpm_discretize = {discretize!r}: one of {DPM_DISCRETIZE}")
    ts = np.unique(np.asarray(ts, dtype=np.int64))    # ascending, repeats dropped
    a = acp[ts]
    a_prev = np.asarray([acp[0]] + acp[ts[:-1]].tolist(), dtype=np.float64)
    return dict(ddim_timesteps=ts, ddim_alphas=a, ddim_alphas_prev=a_prev,
                ddim_sqrt_one_minus_alphas=np.sqrt(1.0 - a.astype(np.float64)).astype(np.float32), ddim_sigmas=np.zeros(len(ts), np.float64),
                lambdas=_log_snr(a), lambdas_prev=_log_snr(a_prev))


def dpm_step_coefs(sched: Dict[str, np.ndarray], index: int, prev_index: Optional[int] = None,
                   order: int = 2, n_nodes: Optional[int] = None) -> Tuple[float, float, float, float, float, float]:
    """The scalars of one DPM-Solver++(2M) step from node ``index`` (a_t) to its a_prev, in float64, each rounded ONCE to float32:
    (sqrt(a_t), sqrt(1 - a_t), c_x, c_d, w1, w0) of

        x0 = (x - s1m * e) / sqrt_at;  D = w1 * x0 + w0 * x0_old;  x_prev = c_x * x + c_d * D

    with h = lambda(a_prev) - lambda(a_t) > 0, c_x = sqrt(1 - a_prev) / sqrt(1 - a_t), c_d = -sqrt(a_prev) * expm1(-h).  ``prev_index``:
    the node of the step before (whose x0 is ``x0_old``), None on the first step.  Second order: r = h_of_that_step / h,
    (w1, w0) = (1 + 1 / (2 r), -1 / (2 r)).  First order, (w1, w0) = (1, 0) -- DDIM with eta 0 in exponential-integrator form: the first step,
    ``order`` 1, and the last step (index 0) of a schedule with fewer than DPM_LOWER_ORDER_FINAL nodes.  ``n_nodes``: the number of nodes that
    run, where that is not the whole schedule (image-to-image runs its last ``img2img_run_steps`` nodes); None = all of them."""
    if order not in DPM_ORDERS:
        raise ValueError(f"dpm_order = {order!r}: one of {DPM_ORDERS}")
    f = np.float32
    n = len(sched["ddim_timesteps"]) if n_nodes is None else int(n_nodes)
    a_t, a_prev = np.float64(sched["ddim_alphas"][index]), np.float64(sched["ddim_alphas_prev"][index])
    h = np.float64(sched["lambdas_prev"][index]) - np.float64(sched["lambdas"][index])
    c_x = np.sqrt(1.0 - a_prev) / np.sqrt(1.0 - a_t)
    c_d = -np.sqrt(a_prev) * np.expm1(-h)
    first_order = prev_index is None or order == 1 or (index == 0 and n < DPM_LOWER_ORDER_FINAL)
    if first_order:
        w1, w0 = 1.0, 0.0
    else:
        r = (np.float64(sched["lambdas_prev"][prev_index]) - np.float64(sched["lambdas"][prev_index])) / h
        w1, w0 = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
    return (float(f(np.sqrt(a_t))), float(f(np.sqrt(1.0 - a_t))), float(f(c_x)), float(f(c_d)), float(f(w1)), float(f(w0)))


IMG2IMG_DEFAULT_STRENGTH = 0.75       # the default of the Stable Diffusion img2img script


def check_strength(v) -> float:
    """``strength`` of image-to-image sampling (SDEdit, Meng et al., arXiv 2108.01073): the share of the schedule that runs on the noised
    input image.  A finite real number in (0, 1] that is no bool, else ValueError naming ``strength``."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not 0 < v <= 1:
        raise ValueError(f"strength = {v!r}: must be a finite number in (0, 1]")
    return float(v)


def img2img_run_steps(n: int, strength: float) -> int:
    """How many of a schedule's ``n`` nodes image-to-image sampling runs -- its last ones: ``t_enc = int(strength * steps)`` of the Stable
    Diffusion img2img script, kept within [1, n]."""
    return max(1, min(int(n), int(check_strength(strength) * int(n))))


def draw_masks_from_boxes(boxes, size):
    """inpaint_mask_func.py:16-41 with randomize_fg_mask / random_add_bg_mask off: per sample a [size, size] mask of ones (1 = keep)
    with every box's rectangle set to 0 (regenerate).  Box coordinates (ltrb, normalised) are scaled in float32 and truncated with
    int(); the rectangle is the python slice [y0:y1, x0:x1], so all-zero, reversed and sub-pixel boxes change nothing and negative
    ends count from the far side.  Returns a CPU float32 torch tensor [B, 1, size, size].

    ``size`` = ``(H, W)`` (this project's extension; the reference function is square only): x0, x1 are int() of the float32 product
    with W, y0, y1 of the product with H -> [B, 1, H, W].  For H == W that is the square function, bit for bit."""
    import torch
    if torch.is_tensor(boxes):
        boxes = boxes.detach().cpu().numpy()
    boxes = np.asarray(boxes, dtype=np.float32)
    H, W = (size, size) if isinstance(size, (int, np.integer)) else (int(v) for v in size)
    scale = np.array([W, H, W, H], np.float32)
    out = np.ones((boxes.shape[0], 1, H, W), np.float32)
    for k, box in enumerate(boxes):
        for bx in box:
            x0, y0, x1, y1 = (int(v) for v in bx * scale)
            out[k, 0, y0:y1, x0:x1] = 0
    return torch.from_numpy(out)
