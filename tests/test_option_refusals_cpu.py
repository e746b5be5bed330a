"""The option checkers refuse and return today what they did before they were rewritten onto shared definitions:
tools/option_refusals.py's default walk (every combination of at most three non-default settings of
check_anonymize_options, check_pitch_options and check_recipe_options) against tests/golden/option_refusals.json, which
the same tool wrote at the commit before the rewrite."""
import hashlib
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_walked_setting_is_refused_or_returned_as_before():
    spec = importlib.util.spec_from_file_location("option_refusals", os.path.join(ROOT, "tools", "option_refusals.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "option_refusals.json")) as f:
        golden = json.load(f)
    now = tool.walk_all()
    assert sum(len(w) for w in now.values()) == golden["cases"] >= 1000
    for name, walk in now.items():
        # the same settings in the same order as the golden walk, so that its indices name these cases
        assert hashlib.sha256("\n".join(walk).encode()).hexdigest() == golden[name]["settings_sha256"], name
        assert len(walk) == len(golden[name]["outcome"]), name
        for (settings, outcome), index in zip(walk.items(), golden[name]["outcome"]):
            assert set(outcome) in ({"exit"}, {"return"}), (name, settings, outcome)
            assert outcome == golden["outcomes"][index], (name, settings, outcome, golden["outcomes"][index])
