"""The reports of anonymize.py: what ``--report_f0``, ``--report_stoi``, ``--report_prosody``, ``--report_mcd`` and
``--report_formants`` add to its JSON line (DESIGN sections 15, 18, 22, 23, 25).  One row of ``REPORTS`` per flag, one
``Report`` per row that is on: the driver scores every batch with each of them, asks each for its keys per utterance
and, at the end, for its summary.
The options are checked by vocoder.check_anonymize_options (vocoder.REPORT_OPTIONS) before anything here runs."""
import collections
import functools

import torch

from . import features, metrics, ops, pitchnorm, vocoder


class Window:
    """The common window of a batch's two waveforms: width, the smaller of their widths; nv int32 [B] on the device,
    the samples of a row that count in both; ref and deg, the input and the output cut to width, fp32 and contiguous;
    frames int32 [B], the Fbank frames of nv, formed when the first report asks for them; f0, the F0 tracks of the pair
    per tracker, kept by f0_tracks."""

    def __init__(self, width, nv, ref, deg):
        self.width, self.nv, self.ref, self.deg = width, nv, ref, deg
        self.f0 = {}

    @functools.cached_property
    def frames(self):
        return metrics.frame_counts(self.nv, self.width)


class Batch:
    """One batch as the reports see it: wavs [B, N], the input, and out [B, *], the waveforms about to be written, on
    the device; lens the relative lengths of wavs; counts the samples written per row."""

    def __init__(self, wavs, lens, out, counts):
        self.wavs, self.lens, self.out, self.counts = wavs, lens, out, counts

    @functools.cached_property
    def window(self):
        """the Window of the pair, formed when the first report asks for it"""
        width = min(self.wavs.shape[1], self.out.shape[1])
        n_in = [int(round(float(v) * self.wavs.shape[1])) for v in self.lens]
        nv = torch.tensor([min(a, b, width) for a, b in zip(n_in, self.counts)], dtype=torch.int32).to(self.out.device)
        return Window(width, nv, self.wavs[:, :width].float().contiguous(), self.out[:, :width].float().contiguous())


def _f0(batch, f0_method, contour_scale):
    """(mean voiced F0 in Hz, voiced share) per row of the output, over the frames of round(lens N) samples, measured
    with the tracker f0_method; in contour mode also the standard deviation of the voiced F0 over those frames (0
    without a voiced frame)"""
    wav, N = batch.out, batch.out.shape[1]
    lens = batch.lens.to(wav.device, torch.float32).contiguous()
    f0 = pitchnorm.f0_track(wav.contiguous(), method=f0_method, lens=lens)
    _, mean, voiced = ops.pitch_ratio(f0, lens, N)
    frames = (pitchnorm.n_valid(lens, N, wav.device).long() // features.HOP + 1).clamp(max=N // features.HOP + 1)
    rep = mean, voiced.double() / frames.double()
    if contour_scale is None:
        return rep
    zero = torch.zeros((), dtype=torch.float64, device=f0.device)
    live = (torch.arange(f0.shape[1], device=f0.device)[None, :] < frames[:, None]) & (f0 > 0)
    n = live.sum(1).clamp(min=1).double()
    m = torch.where(live, f0.double(), zero).sum(1) / n
    var = torch.where(live, (f0.double() - m[:, None]) ** 2, zero).sum(1) / n
    return rep + (var.sqrt(),)


def _stoi(batch):
    w = batch.window
    s, e, _, segments = ops.stoi(w.ref, w.deg, w.nv)
    return s, e, segments


def f0_tracks(window, f0_method="yin"):
    """the F0 tracks of window.ref and window.deg over the samples that count, tracked once per window and tracker"""
    if f0_method not in window.f0:
        rel = (window.nv.double() / window.width).float()
        window.f0[f0_method] = tuple(pitchnorm.f0_track(w, method=f0_method, lens=rel)
                                     for w in (window.ref, window.deg))
    return window.f0[f0_method]


def _prosody(batch, f0_method, prosody_max_lag):
    w = batch.window
    return ops.f0_compare(*f0_tracks(w, f0_method), w.frames, max_lag=prosody_max_lag)


def _mcd(batch, mcd_band, mcd_order):
    w = batch.window
    return metrics.mel_cepstral_distortion(w.ref, w.deg, w.nv, order=mcd_order, band=mcd_band)


def _formants(batch, f0_method):
    w = batch.window
    return metrics.formant_shift(w.ref, w.deg, w.nv, *f0_tracks(w, f0_method), w.frames)


# options: the settings the scoring call takes by name, with their defaults; score: Batch, **options -> a tuple of
# device tensors [B], the columns; stats: the class that keeps the running means and the columns its append takes;
# keys: per utterance (name, column, the column whose 0 makes it null or None, int or float), a key past the columns
# returned left out; summary: (name in the final object, name in stats.summarize())
Row = collections.namedtuple("Row", "options score stats keys summary")
REPORTS = {                                                 # in the order of the JSON line's keys
    "report_f0": Row({"f0_method": "yin", "contour_scale": None}, _f0, None,
                     (("f0_mean_hz", 0, None, float), ("voiced_share", 1, None, float), ("f0_std_hz", 2, None, float)),
                     ()),
    "report_stoi": Row({}, _stoi, (metrics.IntelligibilityStats, (0, 1, 2)),
                       (("stoi", 0, 2, float), ("estoi", 1, 2, float), ("stoi_segments", 2, None, int)),
                       (("stoi_mean", "stoi"), ("estoi_mean", "estoi"))),
    # columns: rho, lag, common, shift, dev, voicing
    "report_prosody": Row({"f0_method": "yin", "prosody_max_lag": vocoder.PROSODY_LAG_DEFAULT}, _prosody,
                          (metrics.ProsodyStats, (0, 2, 4, 5)),
                          (("f0_corr", 0, 2, float), ("f0_dev_st", 4, 2, float), ("f0_shift_st", 3, None, float),
                           ("f0_lag_frames", 1, None, int), ("f0_common_frames", 2, None, int),
                           ("voicing_agreement", 5, None, float)),
                          (("f0_corr_mean", "f0_corr"), ("f0_dev_st_mean", "f0_dev_st"),
                           ("voicing_agreement_mean", "voicing_agreement"), ("prosody_scored", "scored"))),
    "report_mcd": Row({"mcd_band": vocoder.MCD_BAND_DEFAULT, "mcd_order": vocoder.MCD_ORDER_DEFAULT}, _mcd,
                      (metrics.CepstralStats, (0, 1, 2)),
                      (("mcd_db", 0, 2, float), ("mcd_sync_db", 1, 2, float), ("mcd_frames", 2, None, int)),
                      (("mcd_mean", "mcd"), ("mcd_sync_mean", "mcd_sync"), ("mcd_scored", "scored"))),
    # columns: med1, med2, med3, r1, r2, r3, shift, common
    "report_formants": Row({"f0_method": "yin"}, _formants, (metrics.FormantStats, (6, 3, 4, 5, 7)),
                           (("f1_hz", 0, 7, float), ("f2_hz", 1, 7, float), ("f3_hz", 2, 7, float),
                            ("f1_shift", 3, 7, float), ("f2_shift", 4, 7, float), ("f3_shift", 5, 7, float),
                            ("formant_shift", 6, 7, float), ("formant_frames", 7, None, int)),
                           (("formant_shift_mean", "formant_shift"), ("f1_shift_mean", "f1_shift"),
                            ("f2_shift_mean", "f2_shift"), ("f3_shift_mean", "f3_shift"),
                            ("formants_scored", "scored"))),
}


class Report:
    """One row of REPORTS at work: score() every batch, keys(i) per utterance of the batch scored last, summary() at
    the end.  score() is collect() and fetch(), which the benches time apart."""

    def __init__(self, flag, settings):
        self.row = REPORTS[flag]
        self.opts = {k: d if settings.get(k) is None else settings[k] for k, d in self.row.options.items()}
        self.stats = self.row.stats[0]() if self.row.stats else None
        self.cols = self.rows = None

    def score(self, ids, batch):
        self.collect(ids, self.row.score(batch, **self.opts))
        self.fetch()

    def collect(self, ids, cols):
        """the columns of a batch into the running means"""
        if self.stats:
            self.stats.append(ids, *(cols[c] for c in self.row.stats[1]))
        self.cols = cols

    def fetch(self):
        """the columns to the host in one copy (fp64 holds the fp32 and the int32 values exactly)"""
        self.rows = torch.stack([v.double() for v in self.cols]).cpu().tolist()

    def keys(self, i):
        return {name: kind(self.rows[col][i]) if gate is None or self.rows[gate][i] else None
                for name, col, gate, kind in self.row.keys if col < len(self.rows)}

    def summary(self):
        tot = self.stats.summarize() if self.row.summary else {}
        return {name: tot[key] for name, key in self.row.summary}


def active(settings):
    """a Report per flag that is on, in the order of REPORTS"""
    return [Report(flag, settings) for flag in REPORTS if settings.get(flag)]
