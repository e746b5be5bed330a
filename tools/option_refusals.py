#!/usr/bin/env python3
"""What the three public option checkers say, setting by setting: vocoder.check_anonymize_options,
pitchnorm.check_pitch_options and mcadams.check_recipe_options are called on enumerated option settings, and each case
is recorded as either the SystemExit text or the returned value.  No GPU.  check_anonymize_options is walked twice:
over the anonymisers' options ("anonymize") and over the reports' ("anonymize_reports").

    python tools/option_refusals.py [--full] [--out FILE]

The default walks every combination of at most three non-default settings; ``--full`` walks the whole product of the
value sets below.  The output is one JSON object: "outcomes", the distinct {"exit": text} | {"return": value} in order
of first appearance; per checker "outcome", the index into them of every case in the order walked, and
"settings_sha256" over the walked settings (compact JSON, one per line), which pins that order; and "cases", the number
walked.  tests/golden/option_refusals.json is the default walk at the commits before the checkers were rewritten;
tests/test_option_refusals_cpu.py holds the present code to it."""
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import speech_anonymization_amd as pkg  # noqa: E402,F401  (registers the package name)
from speech_anonymization_amd import mcadams, pitchnorm, vocoder  # noqa: E402

ABSENT = object()
# the first value of every axis is its default; an axis may set several keys at once
ENVELOPE = [(("formant_ratio",), [ABSENT, 1.15, 3.0]),
            (("preserve_formants",), [ABSENT, True]),
            (("lifter",), [ABSENT, 30, 0]),
            (("phase",), [ABSENT, "vocoder", "x"]),
            (("contour_scale",), [ABSENT, 0.5, 3]),
            (("contour_smooth",), [ABSENT, 2]),
            (("f0_method",), [ABSENT, "viterbi", "x"])]
MCADAMS = [(("mcadams",), [ABSENT, 0.8]),
           (("mcadams_min", "mcadams_max"), [ABSENT, (0.5, 0.9)])]
RUN = [(("hip_graph",), [ABSENT, True]),
       (("WORLD_SIZE",), [ABSENT, "2"])]
AXES = {
    "anonymize": [(("pitch_norm",), [ABSENT, True])] + ENVELOPE + MCADAMS + [
        (("recon_ckpt",), [ABSENT, "d"]),
        (("passthrough",), [ABSENT, True]),
        (("report_f0",), [ABSENT, True]),
        (("model_type",), ["convae", "zz"])],
    # the recipes: the keys each checker reads (for the pitch recipe also the target and the yaml's own block, which
    # the top-level settings override), the graph flag and a second rank
    "pitch_recipe": ENVELOPE + [
        (("pitch_target_hz",), [ABSENT, 120.0, 500.0]),
        (("pitch_norm",), [ABSENT, {"phase": "vocoder", "contour_scale": 1.0, "lifter": 20, "r_min": 0.6},
                           {"f0_method": "x", "r_max": 3.0}])] + RUN,
    "mcadams_recipe": MCADAMS + [
        (("mcadams_options",), [ABSENT, {"alpha_min": 0.6, "alpha_max": 0.7, "seed": 5}, {"alpha": 2.0}])] + RUN,
    # the reports of anonymize.py: every flag, its dependent options, and what the flags are checked against
    "anonymize_reports": [
        (("report_stoi",), [ABSENT, True, "yes"]),
        (("report_prosody",), [ABSENT, True, False, "yes"]),
        (("prosody_max_lag",), [ABSENT, 4, 33, True]),
        (("report_mcd",), [ABSENT, True, "yes"]),
        (("mcd_band",), [ABSENT, 8, 64]),
        (("mcd_order",), [ABSENT, 12, 0]),
        (("sample_rate",), [ABSENT, 8000]),
        (("f0_method",), [ABSENT, "viterbi"]),
        (("mcadams",), [ABSENT, 0.8])],
}
BASE = {"anonymize": {"out_dir": "o", "synthetic": 2}, "pitch_recipe": {}, "mcadams_recipe": {}}
BASE["anonymize_reports"] = BASE["anonymize"]
CHECKERS = {"anonymize": vocoder.check_anonymize_options, "pitch_recipe": pitchnorm.check_pitch_options,
            "mcadams_recipe": mcadams.check_recipe_options, "anonymize_reports": vocoder.check_anonymize_options}


def choices(axes, full):
    """tuples of one value index per axis: the whole product, or every one with at most three non-defaults"""
    if full:
        yield from itertools.product(*(range(len(values)) for _, values in axes))
        return
    for k in range(4):
        for where in itertools.combinations(range(len(axes)), k):
            for picked in itertools.product(*(range(1, len(axes[a][1])) for a in where)):
                choice = [0] * len(axes)
                for a, v in zip(where, picked):
                    choice[a] = v
                yield tuple(choice)


def settings_of(axes, choice):
    settings = {}
    for (keys, values), v in zip(axes, choice):
        if values[v] is not ABSENT:
            settings.update(zip(keys, values[v] if len(keys) > 1 else (values[v],)))
    return settings


def walk(name, full=False):
    """{settings as JSON: outcome} of one checker; nothing is skipped and nothing but SystemExit is caught"""
    out = {}
    for choice in choices(AXES[name], full):
        given = settings_of(AXES[name], choice)
        settings = dict(BASE[name], **given)
        environ = {"WORLD_SIZE": settings.pop("WORLD_SIZE")} if "WORLD_SIZE" in settings else {}
        try:
            outcome = {"return": CHECKERS[name](settings, {}, environ)}
        except SystemExit as e:
            outcome = {"exit": str(e)}
        out[json.dumps(given, sort_keys=True, separators=(",", ":"))] = json.loads(json.dumps(outcome))
    return out


def walk_all(full=False):
    return {name: walk(name, full) for name in AXES}


def packed(walks):
    """the walks of walk_all as the object that is written: every distinct outcome once, an index per case"""
    outcomes, res = [], {"cases": sum(len(w) for w in walks.values())}
    for name, w in walks.items():
        index = []
        for outcome in w.values():
            if outcome not in outcomes:
                outcomes.append(outcome)
            index.append(outcomes.index(outcome))
        res[name] = {"settings_sha256": hashlib.sha256("\n".join(w).encode()).hexdigest(), "outcome": index}
    return dict(res, outcomes=outcomes)


def main(argv):
    res = packed(walk_all("--full" in argv))
    rows = [f'"cases": {res["cases"]}'] + [f"{json.dumps(name)}: {json.dumps(res[name])}" for name in AXES]
    rows.append('"outcomes": [\n' + ",\n".join(json.dumps(o) for o in res["outcomes"]) + "\n]")
    text = "{\n" + ",\n".join(rows) + "\n}\n"
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print(f"{res['cases']} cases", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
