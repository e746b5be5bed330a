"""The four reports of anonymize.py together (speech_anonymization_amd/reports.py): what one run with every report flag
prints is, key by key, what four runs with one flag each print, in the documented order, and no report changes a WAV.

The manifest is the glide and the vibrato row of tests/contour_ref.py cut to 16037 and 12000 samples: the second row is
shorter than the batch (lens < 1), and the first is no multiple of the hop, so that ``--passthrough true`` writes 16000
samples of it -- an output narrower than its input, scored over the common width.  Everything is compared with ==:
the same kernels run on the same tensors whichever other reports are on."""
import pytest

from tests import anon_cli

DEV = "cuda:0"
gpu = pytest.mark.gpu
CUTS = (16037, 12000)
FLAGS = ("report_f0", "report_stoi", "report_prosody", "report_mcd")
# the documented order: the mode's keys, then the keys of f0, stoi, prosody and mcd
UTT_ORDER = ["id", "spectral_convergence", "samples", "peak", "f0_mean_hz", "voiced_share", "stoi", "estoi",
             "stoi_segments", "f0_corr", "f0_dev_st", "f0_shift_st", "f0_lag_frames", "f0_common_frames",
             "voicing_agreement", "mcd_db", "mcd_sync_db", "mcd_frames"]
LINE_ORDER = ["out_dir", "model_type", "passthrough", "recon_ckpt", "n_iter", "seed", "utterances", "stoi_mean",
              "estoi_mean", "f0_corr_mean", "f0_dev_st_mean", "voicing_agreement_mean", "prosody_scored", "mcd_mean",
              "mcd_sync_mean", "mcd_scored"]


def _held_by_one(both, singles, where):
    """every key of ``both`` that is not in all of ``singles`` (the mode's own, which must agree) is in exactly one"""
    for key, value in both.items():
        holders = [flag for flag, single in singles.items() if key in single]
        if len(holders) == len(singles):
            if key not in ("out_dir", "utterances"):
                assert all(single[key] == value for single in singles.values()), (where, key)
            continue
        assert len(holders) == 1, (where, key, holders)
        assert singles[holders[0]][key] == value, (where, key, singles[holders[0]][key], value)


@gpu
def test_reports_together_print_what_each_prints_alone(tmp_path, capsys):
    from tests import contour_ref as Cr
    rows = [row[:n] for row, n in zip(Cr.case_rows(), CUTS)]
    csv = anon_cli.manifest(tmp_path, anon_cli.ROWS, rows)

    def run(name, flags):
        out = tmp_path / name
        argv = ["--device", DEV, "--csv", csv, "--out_dir", str(out), "--passthrough", "true", "--n_iter", "2"]
        for flag in flags:
            argv += [f"--{flag}", "true"]
        res = anon_cli.run(capsys, argv)
        return res, {name: (out / f"{name}.wav").read_bytes() for name in anon_cli.ROWS}

    both, wavs = run("all", FLAGS)
    singles = {}
    for flag in FLAGS:
        singles[flag], alone = run(flag, (flag,))
        assert alone == wavs, flag
    assert list(both) == LINE_ORDER
    ids = [u["id"] for u in both["utterances"]]
    assert sorted(ids) == sorted(anon_cli.ROWS)
    assert all([u["id"] for u in single["utterances"]] == ids for single in singles.values())
    assert both["utterances"][ids.index("glide")]["samples"] == 16000 < CUTS[0]     # narrower than its input
    _held_by_one(both, singles, "line")
    for i, u in enumerate(both["utterances"]):
        assert list(u) == UTT_ORDER, u["id"]
        _held_by_one(u, {flag: single["utterances"][i] for flag, single in singles.items()}, u["id"])
