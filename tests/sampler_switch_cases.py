"""The grid of the sampler-switch golden (tests/golden/sampler_switch.json): every combination of the per-call keys, valid and not.  Shared by
tools/make_sampler_switch_golden.py, which records what the switch answers, and tests/test_sampler_switch_host.py, which replays it."""
import itertools

KEYS = ("sampler", "ddim_eta", "ddim_discretize", "dpm_order", "dpm_discretize")
AXES = (
    ("plms", "ddim", "dpmpp_2m", "euler", None),
    (0.0, 0.5, -1, float("nan"), True, "0"),
    ("uniform", "quad", "cubic"),
    (2, 1, 3, True, 2.0),
    ("logsnr", "quad", "uniform", "karras"),
)


def rows():
    """the grid in its recorded order: one dict of the five keys per row"""
    return [dict(zip(KEYS, combo)) for combo in itertools.product(*AXES)]


def outcome(fn):
    """what a call answers, in the golden's form: ["ok", repr of each returned value] or ["raises", exception type, full message]"""
    try:
        return ["ok"] + [repr(v) for v in fn()]
    except Exception as e:      # noqa: BLE001  (the type is part of the record)
        return ["raises", type(e).__name__, str(e)]
