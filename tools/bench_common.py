"""What the tools/*_bench.py files share: how a call is timed and how the result line leaves."""
import json
import os
import statistics

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_calls(fn, warmup, steps):
    """the median over ``steps`` calls of the device time of one, events around each, after ``warmup`` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def bench_brain(script, batch_size, scratch, overrides=None, plain=False):
    """the brain of the gender-classifier recipe ``script`` (a key of gender.RECIPES, the script's name) on its own
    YAML, on cuda:0 and ready for fit_batch: built through the script's row (its checker, its transforms, its brain
    class), with ``overrides`` as the command line would give them, logs under ``scratch`` and no checkpointer.
    ``plain``: the plain recipe's row on the same settings, which the step_plain_ms figures time"""
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    stem = "gender_classifier_train"
    if script not in gender.RECIPES:
        raise ValueError(f"bench_brain: {script!r} is no recipe; one of {', '.join(gender.RECIPES)}")
    row = gender.RECIPES[stem if plain else script]
    with open(os.path.join(ROOT, "speechbrain_configs", "gender_classifier" + script[len(stem):] + ".yaml")) as f:
        st = load_hyperpyyaml(f, dict({"output_folder": scratch, "batch_size": batch_size}, **(overrides or {})))
    b, _ = gender.recipe_brain(row, st, {"device": "cuda:0"}, row.check(st, {}, {}) if row.check else None,
                               checkpointer=False)
    b.on_fit_start()
    b.modules.train()
    return b


def write_line(res, out):
    """prints ``res`` as one JSON line and, if ``out`` names a file, writes the line there"""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
