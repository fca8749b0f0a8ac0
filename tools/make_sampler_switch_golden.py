#!/usr/bin/env python3
"""Record what the sampler switch answers on the whole grid of tests/sampler_switch_cases.py into tests/golden/sampler_switch.json:
``interface.check_sampler_args`` followed by ``interface.check_dpm_args``, chained the way ``interface._run`` chains them.  Per row either the
five returned values (as ``repr``, so that 1 and 1.0 differ) or the exception's type and full message.

    python tools/make_sampler_switch_golden.py

Run it on the commit whose answers are to be kept; tests/test_sampler_switch_host.py replays the grid against the file.  The file holds the
distinct outcomes once and one index per row, in grid order.
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import sampler_switch_cases as sc  # noqa: E402

from layoutllm_t2i_amd import interface as itf  # noqa: E402


def chained(sampler, ddim_eta, ddim_discretize, dpm_order, dpm_discretize):
    sampler_args = itf.check_sampler_args(sampler, ddim_eta, ddim_discretize)
    return sampler_args + itf.check_dpm_args(sampler_args[0], dpm_order, dpm_discretize, *sampler_args[1:])


def main():
    outcomes, index = [], []
    for row in sc.rows():
        o = sc.outcome(lambda: chained(**row))
        if o not in outcomes:
            outcomes.append(o)
        index.append(outcomes.index(o))
    path = os.path.join(REPO, "tests", "golden", "sampler_switch.json")
    with open(path, "w") as f:
        top = dict(keys=list(sc.KEYS), axes=[[repr(v) for v in axis] for axis in sc.AXES], outcomes=outcomes, rows=index)
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in top.items()) + "\n}\n")      # one top-level key per line
    print(f"{len(index)} rows, {len(outcomes)} distinct outcomes -> {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
