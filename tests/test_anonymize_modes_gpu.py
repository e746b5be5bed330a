"""Every mode of anonymize.py through its one driver loop: the keys of the final JSON object and of its utterances, in
the order each mode has always printed them, and ``samples`` against the WAV file written.  Three utterances of one
second are the smallest input with a batch, a relative length below 1 and STOI's 30 frames."""
import os

import pytest

from tests import anon_cli

DEV = "cuda:0"
gpu = pytest.mark.gpu

REPORTS = ["f0_mean_hz", "voiced_share", "stoi", "estoi", "stoi_segments"]
MEANS = ["stoi_mean", "estoi_mean"]
PITCH_HEAD = ["out_dir", "pitch_norm", "pitch_target_hz", "n_iter", "seed", "utterances"]
MCADAMS_UTT = ["id", "samples", "peak", "alpha", "gain", "silent_frames", "fallback_frames"] + REPORTS
# mode -> (its flags, the keys of the final object, the keys of every utterance)
MODES = {
    "passthrough": (["--passthrough", "true"],
                    ["out_dir", "model_type", "passthrough", "recon_ckpt", "n_iter", "seed", "utterances"] + MEANS,
                    ["id", "spectral_convergence", "samples", "peak"] + REPORTS),
    "pitch_norm": (["--pitch_norm", "true"], PITCH_HEAD + MEANS, ["id", "samples", "peak", "ratio"] + REPORTS),
    "contour": (["--pitch_norm", "true", "--phase", "vocoder", "--contour_scale", "0.5", "--f0_method", "viterbi"],
                PITCH_HEAD + ["phase", "contour_scale", "contour_smooth", "f0_method"] + MEANS,
                ["id", "samples", "peak", "ratio", "f0_mean_hz", "voiced_share", "f0_std_hz", "stoi", "estoi",
                 "stoi_segments"]),
    "formant_shift": (["--formant_ratio", "1.15"],
                      ["out_dir", "formant_shift", "n_iter", "seed", "utterances", "formant_ratio"] + MEANS,
                      ["id", "samples", "peak"] + REPORTS),
    "mcadams": (["--mcadams", "0.8"], ["out_dir", "mcadams", "utterances", "seed", "level", "alpha"] + MEANS,
                MCADAMS_UTT),
    "mcadams_range": (["--mcadams_min", "0.5", "--mcadams_max", "0.9"],
                      ["out_dir", "mcadams", "utterances", "seed", "level", "alpha_range"] + MEANS, MCADAMS_UTT),
}


@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_every_mode_prints_its_keys_and_writes_its_samples(mode, tmp_path, capsys):
    from speech_anonymization_amd import data
    flags, top, per_utterance = MODES[mode]
    res = anon_cli.run(capsys, ["--device", DEV, "--out_dir", str(tmp_path), "--synthetic", "3", "--batch_size", "3",
                                "--n_iter", "2", "--report_f0", "true", "--report_stoi", "true"] + flags)
    assert list(res) == top
    assert [u["id"] for u in res["utterances"]] == [f"synthetic_{i:04d}" for i in range(3)]
    assert sorted(os.listdir(tmp_path)) == [f"synthetic_{i:04d}.wav" for i in range(3)]
    for u in res["utterances"]:
        assert list(u) == per_utterance, u
        assert data.read_audio(os.path.join(tmp_path, u["id"] + ".wav")).numel() == u["samples"] > 0, u
