"""anonymize.py as the GPU tests run it: in this process (``run``) or in a fresh child (``run_child``); both return the
JSON object of its last line.  ``manifest`` writes waveforms as a manifest for it; ``child`` runs it on the glide and
the vibrato row of tests/contour_ref.py."""
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


def manifest(tmp_path, names, rows):
    """rows (one waveform each) as 16-bit files named by ``names`` and a four-column manifest -> its path"""
    from speech_anonymization_amd import data
    lines = ["ID,duration,wav,gender"]
    for name, row in zip(names, rows):
        path = tmp_path / f"{name}.wav"
        data.write_audio(str(path), row)
        lines.append(f"{name},{row.shape[0] / 16000.0},{path},M")
    csv = tmp_path / "rows.csv"
    csv.write_text("\n".join(lines) + "\n")
    return str(csv)


ROWS = ("glide", "vibrato")


def child(tmp_path, name, extra):
    """a fresh child on the glide and the vibrato row -> (its JSON object, its utterances by id)"""
    from tests import contour_ref as Cr
    res = run_child(["--device", "cuda:0", "--csv", manifest(tmp_path, ROWS, Cr.case_rows()), "--out_dir",
                     str(tmp_path / name)] + extra)
    return res, {u["id"]: u for u in res["utterances"]}
