"""Evaluation-side bookkeeping of the reference's hooks (speechbrain_convae_train.py:130-149,278-306):

  * ``AccuracyStats``            -- speechbrain.utils.Accuracy.AccuracyStats as the reference uses it
                                    (``append(log_probs.unsqueeze(0), labels.unsqueeze(0), length)``,
                                    ``summarize()`` = correct / total), counted on the device;
  * ``SimilarityMetricsStats``   -- utils/utility_similarity_aggregator.py:4-53 (running sum of the
                                    per-utterance encoder cosine similarities: "Utility_Retention").
"""
import torch


class AccuracyStats:
    def __init__(self):
        self.correct = 0
        self.total = 0

    def append(self, log_probabilities, targets, length=None):
        """log_probabilities [..., classes]; targets [...] (the reference passes both with a leading
        singleton batch axis and `length` = the number of utterances, which selects all of them)."""
        pred = log_probabilities.argmax(dim=-1).reshape(-1)
        tgt = torch.as_tensor(targets, device=pred.device).reshape(-1)
        self.correct = self.correct + (pred == tgt).sum()
        self.total += int(tgt.numel())

    def summarize(self):
        return float(self.correct) / max(1, self.total)


class SimilarityMetricsStats:
    def __init__(self):
        self.clear()

    def clear(self):
        self.scores, self.summary = [], {}
        self.value, self.denom = 0, 0

    def append(self, scores):
        scores = scores.detach()
        self.scores.extend(scores)
        self.value = self.value + torch.sum(scores)
        self.denom += scores.shape[0]

    def peek(self):
        return self.value / (1.0 * self.denom)

    def summarize(self):
        if isinstance(self.scores, list):
            self.scores = torch.stack(self.scores)
        self.summary["average"] = torch.sum(self.scores) / self.scores.shape[0]
        return self.summary["average"]


class _GatedMeans:
    """Per-utterance scores of a set of utterances, accumulated on the device in fp64: the columns named in ``gated``
    are averaged over the rows that could be scored (gate > 0), those in ``ungated`` over all rows; the rows that
    could not be scored are counted apart.  summarize() gives one key per column, then scored and unscored."""
    gated, ungated = (), ()

    def __init__(self):
        self.clear()

    def clear(self):
        self.ids = []
        self.sums, self.scored, self.total = dict.fromkeys(self.gated + self.ungated, 0.0), 0, 0

    def _add(self, ids, gate, *columns):
        """gate int [B]; columns fp32 [B], the gated ones and then the ungated ones (tensors, on any one device)"""
        ok = gate.detach() > 0
        zero = torch.zeros((), dtype=torch.float64, device=ok.device)
        self.ids.extend(ids)
        for name, v in zip(self.sums, columns):
            v = v.detach().double()
            self.sums[name] = self.sums[name] + (torch.where(ok, v, zero) if name in self.gated else v).sum()
        self.scored = self.scored + ok.sum()
        self.total += int(ok.numel())

    def summarize(self):
        n = int(self.scored)
        return dict({name: float(v) / d if d else None for name, v in self.sums.items()
                     for d in (n if name in self.gated else self.total,)}, scored=n, unscored=self.total - n)


class IntelligibilityStats(_GatedMeans):
    """STOI / ESTOI of a set of utterances (ops.stoi): the means over the rows with segments > 0"""
    gated = ("stoi", "estoi")

    def append(self, ids, stoi, estoi, segments):
        """ids: a sequence of B names; stoi, estoi fp32 [B]; segments int [B] (tensors, on any one device)"""
        self._add(ids, segments, stoi, estoi)


class ProsodyStats(_GatedMeans):
    """Pitch correlation of a set of utterances (ops.f0_compare): the means of the correlation and
    of the deviation over the rows with common > 0, the mean of the voicing agreement over all rows"""
    gated, ungated = ("f0_corr", "f0_dev_st"), ("voicing_agreement",)

    def append(self, ids, rho, common, dev_st, voicing):
        """ids: a sequence of B names; rho, dev_st, voicing fp32 [B]; common int [B] (tensors, on any one device)"""
        self._add(ids, common, rho, dev_st, voicing)


class CepstralStats(_GatedMeans):
    """Mel-cepstral distortion of a set of utterances (ops.mcd): the means over the rows with
    frames > 0"""
    gated = ("mcd", "mcd_sync")

    def append(self, ids, mcd, mcd_sync, frames):
        """ids: a sequence of B names; mcd, mcd_sync fp32 [B]; frames int [B] (tensors, on any one device)"""
        self._add(ids, frames, mcd, mcd_sync)


class FormantStats(_GatedMeans):
    """Formant shifts of a set of utterances (ops.formant_compare): the means of the geometric-mean
    ratio and of the three per-formant ratios over the rows with common > 0"""
    gated = ("formant_shift", "f1_shift", "f2_shift", "f3_shift")

    def append(self, ids, shift, r1, r2, r3, common):
        """ids: a sequence of B names; shift, r1, r2, r3 fp32 [B]; common int [B] (tensors, on any one device)"""
        self._add(ids, common, shift, r1, r2, r3)


def frame_counts(n_valid, width):
    """n_valid int32 [B], the samples of a row that count, of ``width`` -> the Fbank frames that count, int32 [B]"""
    from . import features
    return (n_valid // features.HOP + 1).clamp(max=width // features.HOP + 1).to(torch.int32)


_fbank = {}


def log_mels(*wavs):
    """wavs [B, N] at 16 kHz on one GPU -> their log-Mel spectra through features.Fbank and its per-utterance clamp at
    amax - 80 dB, contiguous"""
    from . import features
    dev = wavs[0].device
    if dev not in _fbank:
        _fbank[dev] = features.Fbank().to(dev)
    return tuple(_fbank[dev](w.float().contiguous()).clamped().contiguous() for w in wavs)


def mel_cepstral_distortion(wav_ref, wav_deg, n_valid, order=13, band=16):
    """wav_ref, wav_deg fp32 [B, N] at 16 kHz on the GPU, already at a common width; n_valid int [B], the samples of a
    row that count -> (mcd fp32 [B], mcd_sync fp32 [B], frames int32 [B]) of ops.mcd: both go
    through log_mels, and the first n_valid // 160 + 1 frames of a row, at most N // 160 + 1, are compared."""
    from . import ops
    frames = frame_counts(n_valid.to(wav_ref.device), wav_ref.shape[1])
    return ops.mcd(*log_mels(wav_ref, wav_deg), frames, frames, order=order, band=band)


def formant_shift(wav_ref, wav_deg, n_valid, f0_ref, f0_deg, frames, min_common=8):
    """wav_ref, wav_deg fp32 [B, N] at 16 kHz on the GPU, already at a common width; n_valid int32 [B], the samples of
    a row that count; f0_ref, f0_deg fp32 [B, N // 160 + 1], their F0 tracks; frames int32 [B], the frames that count
    -> the columns of ops.formant_compare: both waveforms are tracked in one launch, as a [2 B, N]
    batch, and wav_deg's formants are read against wav_ref's on the frames voiced in both."""
    from . import ops
    B = wav_ref.shape[0]
    F, st = ops.formant_tracks(torch.cat((wav_ref, wav_deg)), torch.cat((n_valid, n_valid)))
    return ops.formant_compare(F[:B], F[B:], st[:B], st[B:], f0_ref, f0_deg, frames, min_common=min_common)
