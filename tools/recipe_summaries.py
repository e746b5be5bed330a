#!/usr/bin/env python3
"""What the eight gender-classifier scripts print, option set by option set, without training: every
gender_classifier_train*.py is loaded by path and its ``main`` called with ``--device cpu --output_folder <tmp>
--synthetic 4`` and the options of CASES, while ``Brain.fit`` and ``Brain.evaluate`` are replaced by stand-ins that leave
``last_stats = {"loss": 0.5, "error": 0.25}``.  Per case the record is every line ``main`` printed (the augmentation
notice and the JSON summary, so the order of its keys), ``max_grad_norm`` as the brain received it, and the SystemExit
text where ``main`` refused.  The temporary folder reads ``<TMP>`` in the record.  No GPU: the transforms are
constructed and never called.

    python tools/recipe_summaries.py [--out FILE]

The recon recipe needs a checkpoint on disk: its cases are its refusals, and one run on an untrained fcae whose
state dict the tool writes into the temporary folder first.  tests/golden/gender_recipe_summaries.json is this tool's
output at the commit before the scripts were put onto gender.run_recipe; tests/test_gender_recipes_cpu.py holds the
present code to it."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import speech_anonymization_amd as pkg  # noqa: E402,F401  (registers the package name)
from speech_anonymization_amd import brain, gender  # noqa: E402

TMP = "<TMP>"
AUGMENT = ["--augment", "true"]
# script and config suffix -> the option sets; a set is the extra arguments, or (the arguments, the environment)
CASES = {
    "": [[], AUGMENT, ["--max_grad_norm", "2.5"]],
    "_pitch_norm": [[], ["--psola", "true"], ["--phase", "vocoder", "--contour_scale", "0.5"],
                    ["--preserve_formants", "true"], ["--formant_ratio", "1.15", "--lifter", "24"],
                    ["--psola", "true", "--contour_scale", "0", "--f0_method", "viterbi"],
                    ["--pitch_target_hz", "120"] + AUGMENT, ["--psola", "true", "--phase", "vocoder"],
                    ["--hip_graph", "true"], ([], {"WORLD_SIZE": "2"})],
    "_mcadams": [[], ["--mcadams", "0.9"], ["--mcadams_min", "0.7", "--mcadams_max", "0.9"], AUGMENT,
                 ["--mcadams", "3"], ["--hip_graph", "true"]],
    "_formant_norm": [[], ["--pitch_norm", "true"], ["--pitch_norm", "true", "--pitch_target_hz", "150"],
                      ["--formant_norm_ratio", "1.1"], ["--formant_norm", "true"], ["--formant_norm", "false"],
                      ["--f0_method", "viterbi", "--pitch_norm", "true"] + AUGMENT, ["--hip_graph", "true"]],
    "_resynth": [[], ["--resynth_pitch_hz", "150"], ["--aspiration", "0.2", "--f0_method", "viterbi"], AUGMENT,
                 ([], {"WORLD_SIZE": "2"})],
    "_modspec": [[], ["--modspec_cutoff_hz", "4", "--modspec_depth", "0.5"], AUGMENT, ["--hip_graph", "true"]],
    "_tempo": [[], ["--tempo", "1.25"], ["--tempo_min", "0.8", "--tempo_max", "1.25"], AUGMENT,
               ["--tempo", "0.8", "--tempo_min", "0.8", "--tempo_max", "1.25"], ([], {"WORLD_SIZE": "2"})],
    "_recon": [[], ["--recon_ckpt", TMP + "/none", "--model_type", "zz"],
               ["--recon_ckpt", TMP + "/none", "--model_type", "fcae", "--hip_graph", "true"],
               (["--recon_ckpt", TMP + "/none", "--model_type", "fcae"], {"WORLD_SIZE": "2"}),
               ["--recon_ckpt", TMP + "/none", "--model_type", "fcae"],
               ["--recon_ckpt", TMP + "/fcae", "--model_type", "fcae"],
               ["--recon_ckpt", TMP + "/fcae", "--model_type", "fcae", "--recon_normalizer", "checkpoint"] + AUGMENT,
               ["--recon_ckpt", TMP + "/fcae", "--model_type", "convae"]],
}


def load_script(suffix):
    name = "gender_classifier_train" + suffix
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_fcae_checkpoint(folder, batch_size):
    """an untrained fully connected anonymiser and a fresh normaliser, in the layout load_anonymiser reads"""
    from speech_anonymization_amd import features
    os.makedirs(folder)
    model = gender.build_anonymiser("fcae", batch_size=batch_size)
    torch.save({"0." + k: v for k, v in model.state_dict().items()}, os.path.join(folder, "model.ckpt"))
    torch.save(features.InputNormalization(norm_type="global").state_dict(), os.path.join(folder, "normalizer.ckpt"))


@contextlib.contextmanager
def stand_ins(seen):
    """Brain.fit and Brain.evaluate replaced for the block; ``seen`` receives what the brain was given"""
    def fit(self, *args, **kwargs):
        seen["max_grad_norm"] = self.max_grad_norm

    def evaluate(self, *args, **kwargs):
        self.last_stats = {"loss": 0.5, "error": 0.25}
    kept = brain.Brain.fit, brain.Brain.evaluate
    brain.Brain.fit, brain.Brain.evaluate = fit, evaluate
    try:
        yield
    finally:
        brain.Brain.fit, brain.Brain.evaluate = kept


def run_case(suffix, case):
    """one call of the script's ``main`` -> {"printed": lines, "max_grad_norm": x | None[, "exit": text]}"""
    args, environ = case if isinstance(case, tuple) else (case, {})
    main = load_script(suffix).main
    with tempfile.TemporaryDirectory() as tmp:
        if any(a == TMP + "/fcae" for a in args):
            write_fcae_checkpoint(os.path.join(tmp, "fcae"), 32)
        argv = [os.path.join(ROOT, "speechbrain_configs", f"gender_classifier{suffix}.yaml"), "--device", "cpu",
                "--output_folder", os.path.join(tmp, "out"), "--synthetic", "4"] + [a.replace(TMP, tmp) for a in args]
        seen, out, kept = {}, io.StringIO(), dict(os.environ)
        os.environ.pop("WORLD_SIZE", None)
        os.environ.update(environ)
        res = {}
        try:
            with stand_ins(seen), contextlib.redirect_stdout(out):
                main(argv)
        except SystemExit as e:
            res["exit"] = str(e).replace(tmp, TMP)
        finally:
            os.environ.clear()
            os.environ.update(kept)
    return dict(printed=out.getvalue().replace(tmp, TMP).splitlines(), max_grad_norm=seen.get("max_grad_norm"), **res)


def case_name(case):
    args, environ = case if isinstance(case, tuple) else (case, {})
    return " ".join([f"{k}={v}" for k, v in environ.items()] + args) or "defaults"


def run_all():
    """{script: {case name: record}}, in the order of CASES"""
    return {"gender_classifier_train" + suffix: {case_name(c): run_case(suffix, c) for c in cases}
            for suffix, cases in CASES.items()}


def main(argv):
    res = run_all()
    text = "{\n" + ",\n".join(
        json.dumps(script) + ": {\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in cases.items()) + "\n}"
        for script, cases in res.items()) + "\n}\n"
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print(f"{sum(len(c) for c in res.values())} cases", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
