"""Digest of the C++ engine's launch sequences on the GPU box, for A/B parity of two builds of the library: a fixed list of tiny-UNet
cases over every mode the engine's launch helpers branch on; per case one line
    <case> launches=<gl_num_launches> pool=<pool_bytes> sha256=<digest of the raw bytes of the output>
One library per process: GLIGEN_HIP_LIB (see _lib.py) selects an A/B build next to the product library.  Two builds with the same launch
sequences over the same kernels print identical lines; any differing line is a difference in orchestration.
    timeout -k 10 240 python tools/engine_digest.py > a.txt && \
    GLIGEN_HIP_LIB=libgligen_hip_parent.so timeout -k 10 240 python tools/engine_digest.py > b.txt && diff a.txt b.txt
(each run under its own time limit, the second only after the first ended clean)
"""
import dataclasses
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from layoutllm_t2i_amd import host, recipe
from layoutllm_t2i_amd.arch import TINY
from layoutllm_t2i_amd.engine import UNetEngine
from layoutllm_t2i_amd.weights import pack_state_dict, random_state_dict

dev = torch.device("cuda:0")
CFGS = {"text": TINY, "text_image": dataclasses.replace(TINY, grounding="text_image"), "inpaint": dataclasses.replace(TINY, inpaint_mode=True),
        "split": dataclasses.replace(TINY, split_weights=True)}
FP16_COPY = {41: 0, 42: 0}
STRICT = {50: 1, 51: 1}
STRICT_NO_W3 = {50: 1, 51: 0}


def case(name, cfg="text", B=2, hw=16, reps=1, t=481.0, fs=1.0, sd=False, graph=True, opts=None, plms=False, extra_bs=0, step=None):
    return dict(name=name, cfg=cfg, B=B, hw=hw, reps=reps, t=t, fs=fs, sd=sd, graph=graph, opts=opts or {}, plms=plms, extra_bs=extra_bs, step=step)


# B = samples of the latent; the conditioning batch is B * reps ([cond ; uncond] with reps = 2)
CASES = [
    case("text_default"),
    case("text_eager", graph=False),
    case("text_fuser_off", fs=0.0),
    case("text_sd_conv", fs=0.0, sd=True),
    case("text_fp16_copy", opts=FP16_COPY),
    case("text_fp16_copy_2b", reps=2, opts=FP16_COPY),
    case("text_2b_shared_prefix", reps=2),
    case("text_2b_per_sample_t", reps=2, t=[981.0, 481.0, 21.0, 1.0]),
    case("text_plms_step", reps=2, plms=True),
    # step: (entry, with its optional operand -- DDIM: noise and pred_x0; DPM: the history of a second-order step)
    case("text_ddim_step", reps=2, step=("ddim", False)),
    case("text_ddim_step_noise_pred_x0", reps=2, step=("ddim", True)),
    case("text_ddim_step_eager_1b", graph=False, step=("ddim", True)),
    case("text_dpmpp_step_first_order", reps=2, step=("dpmpp", False)),
    case("text_dpmpp_step_second_order", reps=2, step=("dpmpp", True)),
    case("text_dpmpp_step_8x8_1b", B=1, hw=8, step=("dpmpp", True)),
    case("text_8x8", B=1, hw=8),
    case("text_rect_16x24", hw=(16, 24)),
    case("text_32x32_third_pass", B=1, hw=32, reps=2),                 # 2B * 32 * 32 = 2048 rows at the first level: option 45's third pass
    case("text_transpose_v", opts={21: 0}),
    case("text_30_rows_unfused_ln2", opts={43: 0, 25: 0}),
    case("text_image_default", cfg="text_image"),
    case("text_image_fuser_off_2b", cfg="text_image", reps=2, fs=0.0),
    case("inpaint_extra_bs1", cfg="inpaint", reps=2, extra_bs=1),
    case("inpaint_extra_per_sample", cfg="inpaint", reps=2, extra_bs=2),
    case("inpaint_fp16_copy", cfg="inpaint", extra_bs=2, opts=FP16_COPY),
    case("split_default", cfg="split"),
    case("split_default_2b_sd_conv", cfg="split", reps=2, fs=0.0, sd=True),
    case("strict_w3_fused_vt", cfg="split", opts=STRICT),               # Bn * N = 512 rows at C = 64: the fused V^T tail
    case("strict_no_w3", cfg="split", opts=STRICT_NO_W3),
    case("strict_w3_8x8_transpose", cfg="split", B=1, hw=8, opts=STRICT),   # 64 rows: below the tail's bound, the transposes
    case("strict_2b_fuser_off_eager", cfg="split", reps=2, fs=0.0, graph=False, opts=STRICT),
    case("strict_rect_16x24", cfg="split", hw=(16, 24), opts=STRICT),
]

engines = {}


def engine(name):
    if name not in engines:
        cfg = CFGS[name]
        P = pack_state_dict(random_state_dict(cfg, dev, seed=0), cfg, dev, None if cfg.inpaint_mode else recipe.sd_first_conv(cfg, 0))
        engines[name] = UNetEngine(P)
    return engines[name]


z = torch.zeros_like
for c in CASES:
    cfg, eng, B, reps = CFGS[c["cfg"]], engine(c["cfg"]), c["B"], c["reps"]
    inp = {k: torch.from_numpy(v) for k, v in recipe.synth_inputs(cfg, B, c["hw"], n_boxes=4, n_rel=3, seed=5).items()}
    eng.clear_options()
    for k, v in c["opts"].items():
        eng.set_option(k, v)
    eng.use_graphs = c["graph"]
    ti = cfg.grounding == "text_image"
    # [cond ; uncond]: the uncond half has the null context and null grounding
    two = (lambda a, null: torch.cat([a, null], 0)) if reps == 2 else (lambda a, null: a)
    emb = inp["text_embeddings" if ti else "positive_embeddings"]
    more = dict(text_masks=two(inp["text_masks"], z(inp["text_masks"])), image_masks=two(inp["image_masks"], z(inp["image_masks"])),
                image_embeddings=two(inp["image_embeddings"], z(inp["image_embeddings"]))) if ti else {}
    eng.set_conditioning(two(inp["context"], inp["uc"]), two(inp["relations"], inp["relations"]), two(inp["boxes"], z(inp["boxes"])),
                         two(inp["masks"], z(inp["masks"])), two(emb, z(emb)), c["hw"], **more)
    x = inp["x"].to(dev).contiguous()
    if cfg.inpaint_mode:
        g = torch.Generator().manual_seed(7)
        eng.set_inpaint_extra(torch.randn((c["extra_bs"], cfg.in_channels + 1) + tuple(x.shape[-2:]), generator=g))
    t = torch.tensor(c["t"]) if isinstance(c["t"], list) else c["t"]
    if c["plms"]:
        g = torch.Generator().manual_seed(11)
        old = [torch.randn(x.shape, generator=g).to(dev) for _ in range(3)]
        coefs, div = host.PLMS_COEFS[3]
        e_out, x_out = torch.empty_like(x), torch.empty_like(x)
        eng.plms_step(x, x, x_out, e_out, [e_out] + old, coefs, div, t, reps, 7.5, c["fs"], c["sd"], *host.step_coefs(host.make_schedule(50, host.alphas_cumprod()), 30))
        out = torch.cat([e_out, x_out], 0)
    elif c["step"]:
        kind, full = c["step"]
        g = torch.Generator().manual_seed(13)
        other = torch.randn(x.shape, generator=g).to(dev)                # DDIM's noise / DPM's x0 of the step before
        x_out, aux = torch.empty_like(x), torch.zeros_like(x)
        ev = dict(t=t, reps=reps, guidance=7.5, fuser_scale=c["fs"], sd_conv=c["sd"])
        if kind == "ddim":
            sq_at, s1m, sq_ap, dirc, sigma = host.ddim_step_coefs(host.make_ddim_schedule(50, host.alphas_cumprod(), "uniform", 1.0), 30)
            eng.ddim_step(x, x_out, **ev, sqrt_at=sq_at, s1m=s1m, sqrt_aprev=sq_ap, dir_coef=dirc, sigma=sigma if full else 0.0,
                          noise=other if full else None, pred_x0=aux if full else None)
        else:
            sched = host.make_dpm_schedule(20, host.alphas_cumprod())
            sq_at, s1m, c_x, c_d, w1, w0 = host.dpm_step_coefs(sched, 10, 11 if full else None)
            aux.copy_(other)                                             # the history buffer: read (second order) and rewritten in place
            eng.dpmpp_step(x, x_out, aux, **ev, sqrt_at=sq_at, s1m=s1m, c_x=c_x, c_d=c_d, w1=w1, w0=w0, x0_old=aux if full else None)
        out = torch.cat([x_out, aux], 0)
    else:
        out = eng.forward(x, t, c["fs"], c["sd"], reps)
        if c["graph"]:
            out = eng.forward(x, t, c["fs"], c["sd"], reps)          # the second call replays the captured graph
    torch.cuda.synchronize()
    digest = hashlib.sha256(out.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    print(f"{c['name']:32s} launches={eng.num_launches()} pool={eng.pool_bytes()} sha256={digest}", flush=True)
