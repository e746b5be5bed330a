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


class IntelligibilityStats:
    """STOI / ESTOI of a set of utterances (ops.stoi), accumulated on the device: the means are
    over the rows that could be scored (segments > 0); the others are counted apart."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.ids = []
        self.stoi_sum, self.estoi_sum, self.scored, self.total = 0.0, 0.0, 0, 0

    def append(self, ids, stoi, estoi, segments):
        """ids: a sequence of B names; stoi, estoi fp32 [B]; segments int [B] (tensors, on any one device)"""
        ok = segments.detach() > 0
        zero = torch.zeros((), dtype=torch.float64, device=ok.device)
        self.ids.extend(ids)
        self.stoi_sum = self.stoi_sum + torch.where(ok, stoi.detach().double(), zero).sum()
        self.estoi_sum = self.estoi_sum + torch.where(ok, estoi.detach().double(), zero).sum()
        self.scored = self.scored + ok.sum()
        self.total += int(ok.numel())

    def summarize(self):
        n = int(self.scored)
        return {"stoi": float(self.stoi_sum) / n if n else None, "estoi": float(self.estoi_sum) / n if n else None,
                "scored": n, "unscored": self.total - n}


class ProsodyStats:
    """Pitch correlation of a set of utterances (ops.f0_compare), accumulated on the device: the
    means of the correlation and of the deviation are over the rows that could be scored (common > 0), the mean of
    the voicing agreement over all rows."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.ids = []
        self.rho_sum, self.dev_sum, self.voicing_sum, self.scored, self.total = 0.0, 0.0, 0.0, 0, 0

    def append(self, ids, rho, common, dev_st, voicing):
        """ids: a sequence of B names; rho, dev_st, voicing fp32 [B]; common int [B] (tensors, on any one device)"""
        ok = common.detach() > 0
        zero = torch.zeros((), dtype=torch.float64, device=ok.device)
        self.ids.extend(ids)
        self.rho_sum = self.rho_sum + torch.where(ok, rho.detach().double(), zero).sum()
        self.dev_sum = self.dev_sum + torch.where(ok, dev_st.detach().double(), zero).sum()
        self.voicing_sum = self.voicing_sum + voicing.detach().double().sum()
        self.scored = self.scored + ok.sum()
        self.total += int(ok.numel())

    def summarize(self):
        n = int(self.scored)
        return {"f0_corr": float(self.rho_sum) / n if n else None, "f0_dev_st": float(self.dev_sum) / n if n else None,
                "voicing_agreement": float(self.voicing_sum) / self.total if self.total else None, "scored": n,
                "unscored": self.total - n}


_fbank = {}


def mel_cepstral_distortion(wav_ref, wav_deg, n_valid, order=13, band=16):
    """wav_ref, wav_deg fp32 [B, N] at 16 kHz on the GPU, already at a common width; n_valid int [B], the samples of a
    row that count -> (mcd fp32 [B], mcd_sync fp32 [B], frames int32 [B]) of ops.mcd: both go
    through features.Fbank and its per-utterance clamp at amax - 80 dB, and the first n_valid // 160 + 1 frames of a
    row, at most N // 160 + 1, are compared."""
    from . import features, ops
    dev = wav_ref.device
    if dev not in _fbank:
        _fbank[dev] = features.Fbank().to(dev)
    mel_ref, mel_deg = (_fbank[dev](w.float().contiguous()).clamped().contiguous() for w in (wav_ref, wav_deg))
    width = wav_ref.shape[1]
    frames = (n_valid.to(dev) // features.HOP + 1).clamp(max=width // features.HOP + 1).to(torch.int32)
    return ops.mcd(mel_ref, mel_deg, frames, frames, order=order, band=band)


class CepstralStats:
    """Mel-cepstral distortion of a set of utterances (ops.mcd), accumulated on the device: the
    means are over the rows that could be scored (frames > 0); the others are counted apart."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.ids = []
        self.mcd_sum, self.sync_sum, self.scored, self.total = 0.0, 0.0, 0, 0

    def append(self, ids, mcd, mcd_sync, frames):
        """ids: a sequence of B names; mcd, mcd_sync fp32 [B]; frames int [B] (tensors, on any one device)"""
        ok = frames.detach() > 0
        zero = torch.zeros((), dtype=torch.float64, device=ok.device)
        self.ids.extend(ids)
        self.mcd_sum = self.mcd_sum + torch.where(ok, mcd.detach().double(), zero).sum()
        self.sync_sum = self.sync_sum + torch.where(ok, mcd_sync.detach().double(), zero).sum()
        self.scored = self.scored + ok.sum()
        self.total += int(ok.numel())

    def summarize(self):
        n = int(self.scored)
        return {"mcd": float(self.mcd_sum) / n if n else None, "mcd_sync": float(self.sync_sum) / n if n else None,
                "scored": n, "unscored": self.total - n}
