"""Host side of the SpecAugment of the ConvAE train step (specaug.py), no GPU: the bicubic table
against torch's own interpolate, the draw ranges, reseeding, the constructor, the loader and the shipped config."""
import os

import pytest
import torch

from tests import specaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(3, 72), (2, 36), (2, 1008), (1, 12)]
F = 8
TABLE_BAR_UNITS = 24.0


def _x(B, T, seed, F=F):
    return torch.randn(B, T, F, generator=torch.Generator().manual_seed(seed)) * 3.0 + 0.5


def _torch_warp(x, c, w):
    T = x.shape[1]
    it = lambda seg, n: torch.nn.functional.interpolate(seg.unsqueeze(1), (n, x.shape[2]), mode="bicubic",
                                                        align_corners=True).squeeze(1)
    return torch.cat([it(x[:, :c], w), it(x[:, c:], T - w)], 1)


def test_table_against_torch_interpolate():
    """the plan's table evaluated in fp64 against F.interpolate(mode="bicubic", align_corners=True) in fp32, over
    (B, T) = (3, 72), (2, 36), (2, 1008), (1, 12), c in {5, T/2, T-6} and every legal w (ten per c, fewer where
    the segment ends cut them).  Unit: 2^-24 * max_o sum_k |w[o][k]| * max |x|.  Measured worst case: 11.94 units
    (T = 36, c = 30; torch's own fp32 accumulation dominates it); the bar is twice that, 24 units (the limit is 64; a wrong tap, clamp or A
    misses by more than 10^4).  w == c reproduces the rows exactly."""
    from speech_anonymization_amd import specaug
    worst_all = 0.0
    for B, T in CASES:
        x = _x(B, T, T)
        for c in sorted({5, T // 2, T - 6}):
            worst = 0.0
            for w in range(c - 5 + 1, c + 5 + 1):
                if not (1 <= w <= T - 1):
                    continue
                plan = specaug.make_plan(B, T, F, c, w)
                y, sw, exact = R.warp64(x, plan)
                ref = _torch_warp(x, c, w)
                unit = R.EPS * float(sw.max()) * float(x.abs().max())
                assert float(sw.max()) <= 1.375 + 1e-6
                worst = max(worst, float((y - ref.double()).abs().max()) / unit)
                if w == c:
                    assert bool(exact.all()) and torch.equal(y.float(), x) and torch.equal(ref, x)
            print(f"T={T} c={c}: worst {worst:.2f} units")
            worst_all = max(worst_all, worst)
    print(f"worst of all cases {worst_all:.2f} units, bar {TABLE_BAR_UNITS}")
    assert TABLE_BAR_UNITS <= 64
    assert worst_all <= TABLE_BAR_UNITS


def test_single_output_row_and_identity_table():
    """n_out == 1 is row 0 of the segment exactly; n_in == n_out is the identity table"""
    from speech_anonymization_amd import specaug
    base, w = specaug.bicubic_table(7, 1)
    assert base.tolist() == [0] and w.tolist() == [[0.0, 1.0, 0.0, 0.0]] and base.dtype == torch.int32
    base, w = specaug.bicubic_table(9, 9)
    assert base.tolist() == list(range(9)) and torch.equal(w, torch.tensor([0.0, 1.0, 0.0, 0.0]).repeat(9, 1))
    assert w.dtype == torch.float32
    x = _x(2, 12, 3)
    plan = specaug.make_plan(2, 12, F, 6, 1)               # the left segment shrinks to one row
    y, _, exact = R.warp64(x, plan)
    assert bool(exact[0]) and torch.equal(y[:, 0].float(), x[:, 0])
    assert torch.equal(_torch_warp(x, 6, 1)[:, 0], x[:, 0])


@pytest.mark.parametrize("T", [1, 7, 10])
def test_short_input_is_the_identity(T):
    """T - window <= window: no warp is drawn and every row is (0, 1, 0, 0) on itself"""
    from speech_anonymization_amd import specaug
    cfg = specaug.settings(freq_mask=False, time_mask=False)
    for seed in range(20):
        plan = specaug.draw_plan(torch.Generator().manual_seed(seed), 2, T, F, cfg)
        assert plan.c is None and plan.w is None
        assert plan.base.tolist() == list(range(T))
        y, _, exact = R.warp64(_x(2, T, 1), plan)
        assert bool(exact.all()) and torch.equal(y.float(), _x(2, T, 1))
    plan = specaug.draw_plan(torch.Generator().manual_seed(0), 2, 11, F, cfg)
    assert plan.c == 5                                      # T = 11: the one legal centre


def test_draw_ranges():
    """500 draws at the reference's settings: c in [window, T - window - 1], w in [c - window + 1, c + window],
    lengths < width, pos + len <= D - 1 whenever D > max(len) (the max over the whole [B, n] draw)"""
    from speech_anonymization_amd import specaug
    cfg = specaug.settings(freq_mask_width=30, time_mask_width=40, replace_with_zero=False)
    gen = torch.Generator().manual_seed(5)
    seen_c, seen_d = set(), set()
    for i in range(500):
        B, T, Fq = 1 + i % 4, (36, 72, 108, 45)[i % 4], (80, 40)[i % 2]
        p = specaug.draw_plan(gen, B, T, Fq, cfg)
        assert 5 <= p.c <= T - 5 - 1 and p.c - 5 + 1 <= p.w <= p.c + 5
        seen_c.add(p.c), seen_d.add(p.w - p.c)
        for lists, D, width in ((p.freq, Fq, 30), (p.time, T, 40)):
            assert len(lists) == B and all(len(row) == 2 for row in lists)
            mx = max(n for row in lists for _, n in row)
            for row in lists:
                for pos, n in row:
                    assert 0 <= n < width and pos >= 0
                    if D > mx:
                        assert pos + n <= D - 1
    assert seen_d == set(range(-4, 6)) and {5, 30}.issubset(seen_c)
    assert not p.zero


def test_reseeding_and_ranks():
    from speech_anonymization_amd import specaug
    """the same (seed, epoch, rank) gives the same plan words; another epoch, rank or seed gives others"""
    words = lambda m: [specaug.draw_plan(m.gen, 3, 72, 80, m.cfg).words() for _ in range(3)]
    a, b = specaug.SpecAugment(seed=11), specaug.SpecAugment(seed=11)
    a.reseed(2, 1), b.reseed(2, 1)
    wa = words(a)
    assert all(torch.equal(u, v) for u, v in zip(wa, words(b)))
    assert not torch.equal(wa[0], wa[1])
    a.reseed(2, 1)
    assert torch.equal(words(a)[0], wa[0])                  # reseeding rewinds
    for epoch, rank in ((3, 1), (2, 0), (2, 2)):
        b.reseed(epoch, rank)
        assert not all(torch.equal(u, v) for u, v in zip(wa, words(b))), (epoch, rank)
    c = specaug.SpecAugment(seed=12)
    c.reseed(2, 1)
    assert not all(torch.equal(u, v) for u, v in zip(wa, words(c)))


def test_plan_words_layout():
    from speech_anonymization_amd import specaug
    cfg = specaug.settings(replace_with_zero=False)
    p = specaug.make_plan(2, 12, 8, 6, 8, freq=[[(1, 2), (2, 3)], []], time=[[(11, 1)], [(0, 0)]], cfg=cfg)
    w = p.words()
    assert w.dtype == torch.int32 and w.numel() == specaug.plan_words(2, 12) == 8 + 8 * 12 + 33 * 2
    assert w[:4].tolist() == [0, 2, 12, 8]
    rows = w[8:8 + 96].view(12, 8)
    assert rows[:, 0].tolist() == p.base.tolist() and rows[:8, 1].tolist() == [0] * 8 and rows[8:, 1].tolist() == [6] * 4
    assert rows[:8, 2].tolist() == [5] * 8 and rows[8:, 2].tolist() == [11] * 4
    assert torch.equal(rows[:, 4:].contiguous().view(torch.float32), p.wt)
    fr = w[104:136].view(2, 8, 2)
    assert fr[0, :2].tolist() == [[1, 2], [2, 3]] and int(fr[0, 2:].abs().sum()) == 0 and int(fr[1].abs().sum()) == 0
    tm = w[136:168].view(2, 8, 2)
    assert tm[0, 0].tolist() == [11, 1]
    assert w[168:].tolist() == [4 * 12, 0]                  # columns 1..4 of utterance 0, all 12 frames
    assert specaug.make_plan(1, 4, 8, cfg=specaug.settings()).words()[0] == 1


def test_constructor_defaults_and_refusals():
    from speech_anonymization_amd import specaug
    import inspect
    sig = inspect.signature(specaug.SpecAugment.__init__).parameters
    want = dict(time_warp=True, time_warp_window=5, time_warp_mode="bicubic", freq_mask=True,
                freq_mask_width=(0, 20), n_freq_mask=2, time_mask=True, time_mask_width=(0, 100), n_time_mask=2,
                replace_with_zero=True)
    assert list(sig)[1:11] == list(want) and all(sig[k].default == v for k, v in want.items())
    m = specaug.SpecAugment(freq_mask_width=30, time_mask_width=40)
    assert m.cfg.freq_mask_width == (0, 30) and m.cfg.time_mask_width == (0, 40)
    with pytest.raises(ValueError, match="bicubic"):
        specaug.SpecAugment(time_warp_mode="bilinear")
    with pytest.raises(ValueError, match="masks per axis"):
        specaug.SpecAugment(n_freq_mask=9)
    with pytest.raises(ValueError, match="masks per axis"):
        specaug.SpecAugment(n_time_mask=9)
    for Fq in (78, 132, 0):
        with pytest.raises(ValueError, match="multiple of 4"):
            specaug.make_plan(2, 36, Fq)
    with pytest.raises(ValueError, match="masks per axis"):
        specaug.make_plan(1, 36, 80, freq=[[(0, 1)] * 9]).words()
    with pytest.raises(ValueError, match="GPU only"):
        m(torch.zeros(2, 36, 80))


def test_yaml_class_and_shipped_config():
    from speech_anonymization_amd import specaug
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    text = ("augmentation: !new:speechbrain.lobes.augment.SpecAugment\n    time_warp: True\n    time_warp_window: 5\n"
            "    time_warp_mode: bicubic\n    freq_mask: True\n    n_freq_mask: 2\n    time_mask: True\n"
            "    n_time_mask: 2\n    replace_with_zero: False\n    freq_mask_width: 30\n    time_mask_width: 40\n")
    aug = load_hyperpyyaml(text)["augmentation"]
    assert isinstance(aug, specaug.SpecAugment)
    assert aug.cfg.freq_mask_width == (0, 30) and aug.cfg.time_mask_width == (0, 40) and not aug.cfg.replace_with_zero
    with open(os.path.join(ROOT, "speechbrain_configs", "convae.yaml")) as f:
        hp = load_hyperpyyaml(f)
    assert hp["spec_augment"] is False and "augmentation" not in hp
    opts = dict(hp["spec_augment_options"])
    assert isinstance(opts.pop("seed"), int)
    assert opts == dict(time_warp=True, time_warp_window=5, time_warp_mode="bicubic", freq_mask=True,
                        freq_mask_width=30, n_freq_mask=2, time_mask=True, time_mask_width=40, n_time_mask=2,
                        replace_with_zero=False)
    built = specaug.SpecAugment(**hp["spec_augment_options"])
    assert built.cfg.freq_mask_width == (0, 30) and "window 5" in built.describe()
