"""The packed-weight table rule the UNet handle and the VAE handle share (csrc/handle.h, gl_weight_table), host side: unique names, offsets
that strictly increase in steps rounded up to 256 bytes, nbytes = numel x (2 or 4), the total, and the index checks of gl_weight_at /
gl_vae_weight_at -- over the UNet families, both values of option key 55, and the VAE decoder and encoder.

Run as a script it prints every table, for an A/B comparison of two builds of the library (one library per process, see _lib.py):
    python tests/test_handle_host.py > a.txt && GLIGEN_HIP_LIB=libgligen_hip_parent.so python tests/test_handle_host.py > b.txt && diff a.txt b.txt
"""
import ctypes
import dataclasses
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kp_cases as kc
import norel_cases as nc
import sp_cases as sc
from layoutllm_t2i_amd import _lib
from layoutllm_t2i_amd.arch import TINY, VAE_TINY, VAEConfig

# name -> (config, option key 55 at creation or None = the process value); the first four are tools/engine_digest.py's CFGS
UNET = {"text": (TINY, None), "text_image": (dataclasses.replace(TINY, grounding="text_image"), None),
        "inpaint": (dataclasses.replace(TINY, inpaint_mode=True), None), "split": (dataclasses.replace(TINY, split_weights=True), None),
        "keypoint": (kc.KP_TINY[3], None), "spatial": (sc.CANNY_TINY, None), "norel": (nc.NR_TINY, None),
        "text_key55_0": (TINY, 0), "text_key55_1": (TINY, 1)}
VAE = {"vae_tiny_dec_key55_0": (VAE_TINY, False, 0), "vae_tiny_dec_key55_1": (VAE_TINY, False, 1), "vae_tiny_enc": (VAE_TINY, True, None),
       "vae_full_dec": (VAEConfig(), False, None)}
HANDLES = list(UNET) + list(VAE)


def _open(name):
    """-> (handle, table reader, weight_at entry, destroy entry)"""
    l = _lib.lib()
    if name in UNET:
        cfg, fold = UNET[name]
        return _lib.create_engine(cfg, fold), _lib.weight_table, l.gl_weight_at, l.gl_destroy
    cfg, encoder, fold = VAE[name]
    return _lib.create_vae(cfg, encoder=encoder, fold_up=fold), _lib.vae_weight_table, l.gl_vae_weight_at, l.gl_vae_destroy


@pytest.mark.parametrize("name", HANDLES)
def test_table_rule(name):
    h, read, at, destroy = _open(name)
    try:
        table, total = read(h)
        assert len(table) > 0 and len({n for n, *_ in table}) == len(table)
        end = 0
        for i, (n, off, nbytes, dtype, shape) in enumerate(table):
            assert off % 256 == 0 and off == end and (i == 0 or off > table[i - 1][1]), n
            assert dtype in (0, 1) and 1 <= len(shape) <= 4 and nbytes == math.prod(shape) * (2 if dtype == 0 else 4) and nbytes > 0, n
            end = off + (nbytes + 255) // 256 * 256
        assert total == end
        info = _lib.WeightInfo()
        assert at(h, -1, ctypes.byref(info)) == -1 and at(h, len(table), ctypes.byref(info)) == -1
        assert at(h, 0, None) == -1 and at(h, len(table) - 1, ctypes.byref(info)) == 0 and info.name.decode() == table[-1][0]
    finally:
        assert destroy(h) == 0


if __name__ == "__main__":
    for name in HANDLES:
        h, read, _, destroy = _open(name)
        table, total = read(h)
        destroy(h)
        print(f"== {name} entries={len(table)} total={total}")
        for row in table:
            print(*row)
