"""Host side of the waveform augmentation (augment.py), no GPU: the resampling tables, the
notch composition, the random plan, the two recipe configs, the CLASS_MAP entries, the label doubling and the
refusal lines."""
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = [os.path.join(ROOT, "speechbrain_configs", n) for n in ("gender_classifier.yaml", "gender_classifier_recon.yaml")]


def test_resampling_tables():
    from speech_anonymization_amd import augment as A
    for speed, want in ((95, (20, 19, 13)), (105, (20, 21, 13))):
        s_in, s_out, W, first, w = A.resample_table(16000, 160 * speed)
        assert (s_in, s_out, W) == want
        assert first.shape == (s_out,) and w.shape == (s_out, W) and w.dtype == torch.float64
        assert (int(first.min()), int(first.max())) == (-6, 13)
        assert float((w.sum(1) - 1).abs().max()) <= 1e-3
    assert A.resample_table(16000, 16000)[:3] == (1, 1, 1)
    assert float(A.resample_table(16000, 16000)[4]) == 1.0
    for L, lo, hi in ((16000, 15200, 16800), (20, 19, 21), (21, 20, 23), (1, 1, 2)):
        assert (A.resampled_length(L, 16000, 15200), A.resampled_length(L, 16000, 16800)) == (lo, hi)
        assert A.resampled_length(L, 16000, 16000) == L


def test_notch_composition():
    """101 taps; count = 0 is the delta exactly; every notch sums to 1 (1e-4 asked, 1e-12 held: lp sums to 1, hp to
    0), and so do the compositions the GPU tests use.  A composition of random centres does NOT always: the cut
    back to 101 taps (speechbrain's same-length convolution) drops the tails of the 201-tap product, so
    sum(h) = 1 - (the mass cut off at each stage), checked here against an independent convolution; over 600
    draws of 1-3 centres, 114 miss 1e-4 and the worst is 3.4e-3.  Symmetry: sinc is even about tap 50, but the
    definition's window is the PERIODIC Blackman window (bw[100 - n] = bw[n + 1]), so a notch is symmetric only up
    to asym(notch) <= D (1 / |sum lp| + 1 / |sum hp|), D = max |bw[n + 1] - bw[n]|, and a composition up to
    asym(a * b) <= asym(a) |b|_1 + |a|_1 asym(b) (the cut [50:151] is symmetric about the centre)."""
    from speech_anonymization_amd import augment as A
    h0 = A.compose_taps([])
    assert h0.shape == (101,) and float(h0[50]) == 1.0 and float(h0.abs().sum()) == 1.0
    assert torch.equal(A.make_plan(1, 8, 100).h, h0.float())
    for centres in ((0.31,), (0.07, 0.52, 0.9), (0.3, 0.7, 0.1)):
        assert abs(float(A.compose_taps(centres).sum()) - 1) <= 1e-4
    n = torch.arange(102, dtype=torch.float64)
    bw = 0.42 - 0.5 * torch.cos(2 * math.pi * n / 101) + 0.08 * torch.cos(4 * math.pi * n / 101)
    D = float((bw[1:] - bw[:-1]).abs().max())
    x = torch.arange(-50, 51, dtype=torch.float64)

    def sums(f):
        s = lambda a: torch.where(a == 0, torch.ones_like(a), torch.sin(a) / torch.where(a == 0, torch.ones_like(a), a))
        return float((s(3 * f * x) * bw[:101]).sum()), float((s(3 * (f + 0.1) * x) * bw[:101]).sum())

    gen = torch.Generator().manual_seed(0)
    for trial in range(30):
        centres = (1e-14 + torch.rand(1 + trial % 3, generator=gen, dtype=torch.float64)).clamp(max=1.0).tolist()
        h = A.compose_taps(centres)
        assert h.shape == (101,) and h.dtype == torch.float64
        asym, l1, own, lost = 0.0, 1.0, h0.clone(), 0.0
        for f in centres:
            g = A.notch(f)
            assert abs(float(g.sum()) - 1) <= 1e-12
            slp, shp = sums(f)
            a_g = D * (1 / abs(slp) + 1 / abs(shp))
            assert float((g - g.flip(0)).abs().max()) <= a_g
            asym, l1 = asym * float(g.abs().sum()) + l1 * a_g, l1 * float(g.abs().sum())
            full = torch.zeros(201, dtype=torch.float64)
            for k in range(101):
                full[k:k + 101] += own[k] * g
            lost += float(full[:50].sum() + full[151:].sum())
            own = full[50:151].clone()
        assert float((h - own).abs().max()) <= 1e-13
        assert abs(float(h.sum()) - (1 - lost)) <= 1e-12
        assert float((h - h.flip(0)).abs().max()) <= asym
        if len(centres) == 1:
            assert abs(float(h.sum()) - 1) <= 1e-4


def test_plan_is_deterministic_and_in_range():
    from speech_anonymization_amd import augment as A
    lens, L = torch.tensor([1.0, 0.61, 0.33, 0.05]), 16000
    seen = set()
    for seed in range(40):
        p = A.draw_plan(torch.Generator().manual_seed(seed), lens, L)
        q = A.draw_plan(torch.Generator().manual_seed(seed), lens, L)
        assert (p.speed, p.centres, p.chunks) == (q.speed, q.centres, q.chunks) and torch.equal(p.snr, q.snr)
        assert torch.equal(p.words(), q.words())
        seen.add(p.speed)
        assert p.speed in (95, 100, 105) and p.R == 8 and p.Lp == A.resampled_length(L, 16000, 160 * p.speed)
        assert 0 <= len(p.centres) <= 3 and all(1e-14 <= f <= 1.0 for f in p.centres)
        assert p.snr.dtype == torch.float32 and bool(((p.snr >= 0) & (p.snr <= 15)).all())
        assert p.w.dtype == torch.float32 and p.h.dtype == torch.float32 and p.first.dtype == torch.int32
        assert len(p.chunks) == 8
        for r, ivs in enumerate(p.chunks):
            assert 0 <= len(ivs) <= 5
            len_r = int(float(lens[r % 4]) * p.Lp)           # chunk starts come from int(lens * L')
            longest = max((e - s for s, e in ivs), default=0)
            for s, e in ivs:
                assert 1000 <= e - s <= 2000 and 0 <= s <= max(0, len_r - longest)
        assert all(s == 0 for s, _ in p.chunks[3] + p.chunks[7])    # 0.05 * L' < 1000: only start 0 is left
    assert seen == {95, 100, 105}
    quiet = A.draw_plan(torch.Generator().manual_seed(1), lens, L, {"noise": False})
    assert quiet.R == 4 and quiet.snr is None and len(quiet.chunks) == 4


def test_plan_words_layout():
    from speech_anonymization_amd import augment as A
    p = A.make_plan(2, 4133, 95, (0.3,), [[(5, 10)], [], [(1, 2), (3, 4)], []], snr=[1.5, 2.5])
    wds = p.words()
    mc = A.MAX_CHUNKS
    o = 19
    assert wds.dtype == torch.int32 and wds.numel() == 19 + 19 * 13 + 101 + 4 * (1 + 2 * mc) + 2
    assert torch.equal(wds[:o], p.first)
    assert torch.equal(wds[o:o + 247].view(torch.float32), p.w.reshape(-1))
    o += 247
    assert torch.equal(wds[o:o + 101].view(torch.float32), p.h)
    o += 101
    table = wds[o:o + 4 * (1 + 2 * mc)].view(4, -1)
    assert table[:, 0].tolist() == [1, 0, 2, 0] and table[0, 1:3].tolist() == [5, 15]
    assert table[2, 1:5].tolist() == [1, 3, 3, 7]
    assert p.snr_offset == wds.numel() - 2 and wds[p.snr_offset:].view(torch.float32).tolist() == [1.5, 2.5]
    from speech_anonymization_amd._lib import SaHipError
    with pytest.raises(SaHipError, match="at most"):
        A.make_plan(1, 100, 100, (), [[(0, 1)] * (mc + 1)]).words()


def test_epoch_reseeding():
    """(seed, epoch) fixes the host draws: a run resumed at an epoch boundary draws what an uninterrupted one does"""
    from speech_anonymization_amd import augment as A
    lens = torch.tensor([1.0, 0.7])
    a, b = A.TrainAugment(seed=5), A.TrainAugment(seed=5)
    a.reseed(1)
    for _ in range(3):
        A.draw_plan(a.gen, lens, 16000, a.cfg)
    a.reseed(2)
    b.reseed(2)
    pa, pb = A.draw_plan(a.gen, lens, 16000, a.cfg), A.draw_plan(b.gen, lens, 16000, b.cfg)
    assert torch.equal(pa.words(), pb.words())
    c = A.TrainAugment(seed=6)
    c.reseed(2)
    seq = lambda m: [A.draw_plan(m.gen, lens, 16000, m.cfg).chunks for _ in range(4)]
    b.reseed(2)
    assert seq(c) != seq(b)


@pytest.mark.parametrize("cfg", CFGS)
def test_configs_and_build(cfg, tmp_path):
    from speech_anonymization_amd import augment as A, gender
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    text = open(cfg).read()
    assert "!" not in text.replace("# ", "")            # plain values, no tags
    with open(cfg) as f:
        st = load_hyperpyyaml(f, {"output_folder": str(tmp_path)})
    assert st["augment"] is False
    o = st["augment_options"]
    assert o == {"speeds": [95, 100, 105], "noise": True, "snr_low": 0, "snr_high": 15, "drop_freq_count_low": 0,
                 "drop_freq_count_high": 3, "drop_chunk_count_low": 0, "drop_chunk_count_high": 5,
                 "drop_chunk_length_low": 1000, "drop_chunk_length_high": 2000}
    assert set(gender.build(st)["modules"]) == {"compute_features", "embedding_model", "classifier", "mean_var_norm"}
    assert "not part of this build" in gender.augment_notice("x", st)
    st["augment"] = True
    m = gender.build(st)["modules"]
    assert set(m) == {"compute_features", "embedding_model", "classifier", "mean_var_norm", "augmentation"}
    aug = m["augmentation"]
    assert isinstance(aug, A.TrainAugment) and aug.seed == st["seed"] and aug.cfg.speeds == (95, 100, 105)
    assert (aug.cfg.snr_low, aug.cfg.snr_high, aug.cfg.noise) == (0, 15, True)
    assert not list(aug.parameters()) and not aug.state_dict()
    line = gender.augment_notice("x", st)
    assert "\n" not in line and "augmentation on" in line and "white" in line and "OpenRIR" in line
    assert "not part of this build" not in line


def test_class_map_entries():
    from speech_anonymization_amd import augment as A
    from speech_anonymization_amd.yaml_loader import CLASS_MAP, Unavailable, load_hyperpyyaml
    assert CLASS_MAP["speechbrain.lobes.augment.TimeDomainSpecAugment"] == "speech_anonymization_amd.augment.TimeDomainSpecAugment"
    assert CLASS_MAP["speechbrain.processing.speech_augmentation.AddNoise"] == "speech_anonymization_amd.augment.AddNoise"
    y = ("aug: !new:speechbrain.lobes.augment.TimeDomainSpecAugment\n    sample_rate: 16000\n    speeds: [95, 100, 105]\n"
         "noise: !new:speechbrain.processing.speech_augmentation.AddNoise\n    snr_low: 0\n    snr_high: 15\n"
         "corrupt: !new:speechbrain.lobes.augment.EnvCorrupt\n    openrir_folder: x\n")
    hp = load_hyperpyyaml(y)
    assert isinstance(hp["aug"], A.TimeDomainSpecAugment) and not hp["aug"].inner.cfg.noise
    assert isinstance(hp["noise"], A.AddNoise) and hp["noise"].inner.cfg.snr_high == 15
    assert hp["noise"].inner.cfg.speeds == (100,) and hp["noise"].inner.cfg.drop_chunk_count_high == 0
    assert isinstance(hp["corrupt"], Unavailable)
    with pytest.raises(ValueError, match="csv_file"):
        A.AddNoise(csv_file="noise.csv")
    with pytest.raises(ValueError, match="probabilities"):
        A.TimeDomainSpecAugment(drop_chunk_prob=0.5)


def test_labels_are_repeated_for_the_doubled_batch():
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.brain import Batch, Stage
    seen = {}

    def cost(logp, label):
        seen["label"], seen["rows"] = label.clone(), logp.shape[0]
        return logp.sum()

    b = gender.GenderBrain(modules={}, hparams={"compute_cost": cost}, run_opts={"device": "cpu"})
    b.on_stage_start(Stage.TRAIN, 1)
    batch = Batch(torch.zeros(4, 8), torch.ones(4), torch.tensor([0, 1, 1, 0]))
    b._aug = (None, 2)
    b.compute_objectives(torch.zeros(8, 1, 2), batch, Stage.TRAIN)
    assert seen["rows"] == 8 and seen["label"].tolist() == [0, 1, 1, 0, 0, 1, 1, 0]
    b.compute_objectives(torch.zeros(4, 1, 2), batch, Stage.VALID)          # never outside TRAIN
    assert seen["label"].tolist() == [0, 1, 1, 0] and (b.n_err, b.n_utt) == (2, 4)
    b._aug = None
    b.compute_objectives(torch.zeros(4, 1, 2), batch, Stage.TRAIN)
    assert seen["label"].tolist() == [0, 1, 1, 0]


def test_stage_gating_and_host_lengths():
    """the module runs at TRAIN only, gets the loader's CPU lengths, and its lengths reach the classifier"""
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.brain import Stage
    calls = []

    class Aug(torch.nn.Module):
        def forward(self, wavs, lens, host_lens=None):
            calls.append(host_lens)
            return torch.cat([wavs, wavs])[:, :5], lens.repeat(2), 2

        def reseed(self, epoch):
            calls.append(("reseed", epoch))

    b = gender.GenderBrain(modules={"augmentation": Aug()}, run_opts={"device": "cpu"})
    b.on_stage_start(Stage.TRAIN, 3)
    b.on_stage_start(Stage.VALID, 3)
    assert calls == [("reseed", 3)]
    host = torch.ones(2)
    b._host_lens = host
    w, l = b.augment(torch.zeros(2, 8), torch.ones(2), Stage.TRAIN)
    assert w.shape == (4, 5) and l.shape == (4,) and calls[-1] is host and b._aug[1] == 2
    w, l = b.augment(torch.zeros(2, 8), torch.ones(2), Stage.VALID)
    assert w.shape == (2, 8) and b._aug is None and len(calls) == 2


def test_refusal_lines(tmp_path):
    from speech_anonymization_amd import augment as A, gender
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    with open(CFGS[0]) as f:
        st = load_hyperpyyaml(f, {"output_folder": str(tmp_path), "augment": True})

    def refused(match, **over):
        with pytest.raises(SystemExit) as e:
            gender.build(dict(st, **over))
        msg = str(e.value)
        assert match in msg and "\n" not in msg, msg

    refused("at most 65535", batch_size=40000)
    refused("speeds", augment_options=dict(st["augment_options"], speeds=[50, 100]))
    refused("speeds", augment_options=dict(st["augment_options"], speeds=[]))
    refused("dropped chunks", augment_options=dict(st["augment_options"], drop_chunk_count_high=9))
    refused("snr_low", augment_options=dict(st["augment_options"], snr_low=20))
    with pytest.raises(ValueError, match="unknown augmentation setting 'speed'"):
        gender.build(dict(st, augment_options={"speed": 95}))
    gender.build(dict(st, batch_size=32767, augment_options=dict(st["augment_options"], speeds=[75, 130])))
    from speech_anonymization_amd._lib import SaHipError
    with pytest.raises(SaHipError, match="GPU only"):
        A.TrainAugment()(torch.zeros(2, 8), torch.ones(2))
