#!/usr/bin/env python3
"""What each signal-processing baseline costs in intelligibility, does to the pitch and moves in the spectral
envelope, on the synthetic set: anonymize.py --synthetic N --report_stoi true --report_f0 true --report_mcd true
--report_formants true once per mode, each a fresh child process, and per mode the mean STOI, ESTOI, voiced-mean F0 and
voiced share of what it wrote, its mean mel-cepstral distortion from the input in dB, along the
alignment (mcd) and frame against frame (mcd_sync), and the mean factor by which its LPC formants
moved, all three together (formant_shift) and one by one (f1_shift, f2_shift, f3_shift).

  passthrough             the vocoder alone: Fbank -> Mel pseudo-inverse -> Griffin-Lim of the original features
  pitch_norm              pitch normalisation to 170 Hz
  pitch_norm_preserve     the same with the formants kept in place
  formant_ratio_1.15      the envelope scaled by 1.15, the pitch untouched
  mcadams_0.8             the McAdams transform, alpha = 0.8
  pitch_norm_pv, pitch_norm_preserve_pv, formant_ratio_1.15_pv
                          the three Griffin-Lim rows with --phase vocoder: the input's own phases carried through
                          
  pitch_norm_psola, pitch_norm_psola_contour
                          pitch normalisation in the time domain (--psola true, TD-PSOLA), with one
                          ratio per utterance and with --contour_scale 1, a ratio per frame
  formant_norm, formant_norm_psola
                          formant normalisation to (550, 1650, 2750) Hz (--formant_norm true), alone
                          and with --pitch_norm true --psola true behind it: both cues at their targets
  resynth, resynth_170    LPC source-filter resynthesis (--resynth true): every frame's envelope under
                          a pulse/noise excitation, at the utterance's own pitch and with --resynth_pitch_hz 170
  modspec_10              modulation-spectrum smoothing (--modspec_cutoff_hz 10): every STFT bin's log
                          magnitude low-pass filtered along time at 10 Hz, the input's phases kept
  tempo_0.8, tempo_1.25   WSOLA time-scale modification (--tempo X): the F0 columns only -- the mode
                          refuses the reports that compare input and output frame against frame, and their columns
                          are null

The synthetic utterances are steady harmonic series in white noise: the table shows that the scorer and the modes
run end to end and how they rank on that material.  It says nothing about real speech; the formant columns in
particular read poles that sit on harmonics, not on resonances, and are a check of the plumbing there.

    python tools/anonymiser_table.py [--synthetic 32]         # one JSON line, also written to --out
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = (("passthrough", ["--passthrough", "true"]),
         ("pitch_norm", ["--pitch_norm", "true"]),
         ("pitch_norm_preserve", ["--pitch_norm", "true", "--preserve_formants", "true"]),
         ("formant_ratio_1.15", ["--formant_ratio", "1.15"]),
         ("mcadams_0.8", ["--mcadams", "0.8"]),
         ("pitch_norm_pv", ["--pitch_norm", "true", "--phase", "vocoder"]),
         ("pitch_norm_preserve_pv", ["--pitch_norm", "true", "--preserve_formants", "true", "--phase", "vocoder"]),
         ("formant_ratio_1.15_pv", ["--formant_ratio", "1.15", "--phase", "vocoder"]),
         ("pitch_norm_psola", ["--pitch_norm", "true", "--psola", "true"]),
         ("pitch_norm_psola_contour", ["--pitch_norm", "true", "--psola", "true", "--contour_scale", "1"]),
         ("formant_norm", ["--formant_norm", "true"]),
         ("formant_norm_psola", ["--formant_norm", "true", "--pitch_norm", "true", "--psola", "true"]),
         ("resynth", ["--resynth", "true"]),
         ("resynth_170", ["--resynth", "true", "--resynth_pitch_hz", "170"]),
         ("modspec_10", ["--modspec_cutoff_hz", "10"]),
         ("tempo_0.8", ["--tempo", "0.8"]),
         ("tempo_1.25", ["--tempo", "1.25"]))
ALIGNED = ["--report_stoi", "true", "--report_mcd", "true", "--report_formants", "true"]   # what a tempo row leaves out


def _mean(vals):
    vals = [v for v in vals if v is not None]
    return sum(vals) / len(vals) if vals else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, default=32)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds, per mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anonymiser_table.json"))
    a = ap.parse_args()
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, flags in MODES:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "anonymize.py"),
                                os.path.join(ROOT, "speechbrain_configs", "convae.yaml"), "--device", a.device,
                                "--synthetic", str(a.synthetic), "--batch_size", str(a.batch_size), "--out_dir",
                                os.path.join(tmp, name), "--report_f0", "true"] +
                               ([] if name.startswith("tempo_") else ALIGNED) + flags,
                               cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                raise SystemExit(f"{name}: anonymize.py ended with {r.returncode}\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            utts = res["utterances"]
            table[name] = {"stoi": res.get("stoi_mean"), "estoi": res.get("estoi_mean"),
                           "scored": sum(1 for u in utts if u.get("stoi_segments", 0) > 0), "utterances": len(utts),
                           "f0_mean_hz": _mean([u["f0_mean_hz"] for u in utts if u["voiced_share"] > 0]),
                           "voiced_share": _mean([u["voiced_share"] for u in utts]),
                           "mcd": res.get("mcd_mean"), "mcd_sync": res.get("mcd_sync_mean"),
                           "mcd_scored": res.get("mcd_scored"),
                           "formant_shift": res.get("formant_shift_mean"), "f1_shift": res.get("f1_shift_mean"),
                           "f2_shift": res.get("f2_shift_mean"), "f3_shift": res.get("f3_shift_mean"),
                           "formants_scored": res.get("formants_scored")}
    line = json.dumps({"synthetic": a.synthetic, "modes": table})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
