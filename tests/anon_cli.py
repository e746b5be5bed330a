"""anonymize.py as the GPU tests run it: in this process (``run``) or in a fresh child (``run_child``); both return the
JSON object of its last line."""
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "speechbrain_configs", "convae.yaml")


def run(capsys, argv):
    spec = importlib.util.spec_from_file_location("anonymize", os.path.join(ROOT, "anonymize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main([CONFIG] + argv)
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def run_child(argv, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "anonymize.py"), CONFIG] + argv, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])
