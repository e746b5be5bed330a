"""The fused waveform augmentation (csrc/sa_augment.hip, augment.py) against an fp64 restatement
of the same formulas, written here (``reference``).  The restatement takes the plan's own fp32 tables, taps and
noise scales cast up, so only accumulation is compared.  One reference and one bar for every case, per element:

    |y - y64| <= (W + 101 + 3) 2^-24 * sum|h| * max_i sum_j |w[i][j]| * max|x_row|

the dot-product rounding bound of the two chained sums and the mix (x_row: the row as staged, after the mix).
Samples the definition makes zero -- chunk interiors, everything for a zero input -- must be == 0.
Every figure is printed before it is asserted."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = 2.0 ** -24
LENS3 = (1.0, 0.61, 0.33)
# test error of tools/gender_augment_cpu_rehearsal.py (this file's restatement, oracle.features, oracle.xvector under
# torch autograd) at the budget of test_recipe_learns_with_augmentation: --synthetic 96 --batch_size 16
# --number_of_epochs 4, seed 1986
E_CPU = 0.0
E_MARGIN = 0.1                       # DESIGN section 9's margin


# ---------------------------------------------------------------------------------------------------
# the fp64 restatement (CPU; also what tools/gender_augment_cpu_rehearsal.py trains on)
# ---------------------------------------------------------------------------------------------------
def reference_scales(wav, noise, lens, snr):
    """(1 - f, g) [B, 2] fp64 from the formula"""
    L = wav.shape[1]
    den = lens.double() * L
    ac, an = wav.double().abs().sum(1) / den, noise.double().abs().sum(1) / den
    f = 1.0 / (10.0 ** (snr.double() / 20.0) + 1.0)
    return torch.stack([1.0 - f, f * ac / (an + 1e-14)], 1)


def reference(wav, lens, plan, noise=None):
    """-> (y64 [R, Lp], rows64 [R, L]: the rows after the noise mix, zero [R, Lp] bool: samples inside a chunk)"""
    x = wav.double().cpu()
    B, L = x.shape
    if plan.R == 2 * B:
        s = reference_scales(x, noise.cpu(), lens.cpu(), plan.snr).float().double()     # rounded once, as stored
        x = torch.cat([x, s[:, :1] * x + s[:, 1:] * noise.double().cpu()])
    n = torch.arange(plan.Lp)
    q, i = n // plan.S_out, n % plan.S_out
    idx = (q * plan.S_in + plan.first.long()[i])[:, None] + torch.arange(plan.W)[None, :]
    ok = (idx >= 0) & (idx < L)
    r = (x[:, idx.clamp(0, L - 1)] * ok * plan.w.double()[i]).sum(-1)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(r, (50, 50))[:, None, :],
                                   plan.h.double().view(1, 1, -1))[:, 0, :]
    zero = torch.zeros(plan.R, plan.Lp, dtype=torch.bool)
    for row, ivs in enumerate(plan.chunks):
        for s0, e0 in ivs:
            zero[row, s0:min(e0, plan.Lp)] = True
    y[zero] = 0.0
    return y, x, zero


def bound(plan, rows64):
    """per-row bar [R, 1]"""
    return ((plan.W + 101 + 3) * EPS * float(plan.h.double().abs().sum())
            * float(plan.w.double().abs().sum(1).max()) * rows64.abs().amax(1, keepdim=True))


def _wav(B, L, lens, seed):
    g = torch.Generator().manual_seed(seed)
    w = 0.3 * torch.randn(B, L, generator=g)
    for b, rel in enumerate(lens):
        w[b, int(round(rel * L)):] = 0.0
    return w


def _check(tag, wav, lens, plan, noise=None):
    from speech_anonymization_amd import augment
    lens_t = torch.tensor(lens, dtype=torch.float32)
    y64, rows, zero = reference(wav, lens_t, plan, noise)
    out = augment.apply_plan(wav.to(DEV), lens_t.to(DEV), plan, None if noise is None else noise.to(DEV))
    torch.cuda.synchronize()
    got = out.cpu()
    assert got.shape == (plan.R, plan.Lp) and got.dtype == torch.float32
    bar = bound(plan, rows)
    err = (got.double() - y64).abs()
    worst = float((err / bar.clamp_min(1e-300)).max())
    print(f"{tag}: R={plan.R} L={plan.L} Lp={plan.Lp} speed={plan.speed} notches={len(plan.centres)} "
          f"max err {float(err.max()):.3e}  worst err/bar {worst:.4f}  zeroed {int(zero.sum())}")
    assert bool((got[zero] == 0).all())
    assert bool((err <= bar).all()), worst
    return got


CENTRES = {0: (), 1: (0.31,), 3: (0.07, 0.52, 0.9)}


# ---------------------------------------------------------------------------------------------------
# the fused pass
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("notches", [0, 1, 3])
@pytest.mark.parametrize("speed", [95, 100, 105])
def test_speeds_and_notch_counts(speed, notches):
    """B = 3, L = 4133 (no multiple of 4, so unaligned rows; three tiles at speed 105), ragged lengths"""
    from speech_anonymization_amd import augment
    plan = augment.make_plan(3, 4133, speed, CENTRES[notches])
    _check(f"speed {speed} notches {notches}", _wav(3, 4133, LENS3, speed + notches), LENS3, plan)


@pytest.mark.parametrize("case", ["none-five-at0", "end-clipped-overlap"])
def test_chunk_plans(case):
    """no chunk, five chunks, one starting at 0; one ending exactly at L', one clipped by L', two overlapping"""
    from speech_anonymization_amd import augment
    Lp = augment.resampled_length(4133, 16000, 15200)
    chunks = {"none-five-at0": [[], [(100, 1000), (1500, 200), (1800, 7), (2047, 3), (3000, 900)], [(0, 1234)]],
              "end-clipped-overlap": [[(Lp - 1100, 1100)], [(Lp - 500, 2000)], [(1000, 1500), (2000, 1200)]]}[case]
    plan = augment.make_plan(3, 4133, 95, CENTRES[1], chunks)
    got = _check(case, _wav(3, 4133, LENS3, 7), LENS3, plan)
    if case == "none-five-at0":
        assert bool((got[0] != 0).any()) and bool((got[2, :1234] == 0).all()) and float(got[2, 1234:1400].abs().max()) > 0
    else:
        assert bool((got[0, Lp - 1100:] == 0).all()) and bool((got[1, Lp - 500:] == 0).all())
        assert bool((got[2, 1000:3200] == 0).all())


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("speed", [95, 100, 105])
def test_width_at_the_tile_size(speed, extra):
    """L' equal to the kernel's tile and one more (a second workgroup for a single sample)"""
    from speech_anonymization_amd import augment
    want = augment.TILE + extra
    new = 16000 * speed // 100
    L = next(n for n in range(want * 16000 // new - 3, want * 16000 // new + 4)
             if augment.resampled_length(n, 16000, new) == want)
    plan = augment.make_plan(2, L, speed, CENTRES[1], [[(want - 3, 10)], []])
    assert plan.Lp == want
    _check(f"tile + {extra}", _wav(2, L, (1.0, 0.5), speed + extra), (1.0, 0.5), plan)


@pytest.mark.parametrize("L", [37, 1])
@pytest.mark.parametrize("speed", [95, 100, 105])
def test_rows_shorter_than_the_filter(speed, L):
    from speech_anonymization_amd import augment
    plan = augment.make_plan(2, L, speed, CENTRES[3], [[], [(0, 1)]])
    _check(f"L {L}", _wav(2, L, (1.0, 1.0), L + speed) + 0.1, (1.0, 1.0), plan)


def test_noise_rows_against_the_reference():
    """R = 2 B with a given noise tensor: clean rows, then (1 - f) wav + g noise over the whole padded row (the
    noise covers the padded tail too), all through resampling, filter and chunks"""
    from speech_anonymization_amd import augment
    wav = _wav(3, 4133, LENS3, 21)
    noise = torch.randn(3, 4133, generator=torch.Generator().manual_seed(22))
    chunks = [[], [(10, 1000)], [], [(0, 1500), (1400, 1000)], [], [(4000, 2000)]]
    plan = augment.make_plan(3, 4133, 105, CENTRES[3], chunks, snr=[0.0, 7.25, 15.0])
    got = _check("noise rows", wav, LENS3, plan, noise)
    tail = int(0.33 * plan.Lp) + 200
    assert float(got[2, tail:].abs().max()) == 0.0                      # the clean row's padded tail stays zero
    assert float(got[5, tail:4000].abs().max()) > 0.0                   # the noisy copy's tail carries noise


def test_zero_input_gives_zeros():
    from speech_anonymization_amd import augment
    plan = augment.make_plan(2, 3000, 95, CENTRES[3])
    out = augment.apply_plan(torch.zeros(2, 3000, device=DEV), torch.ones(2, device=DEV), plan)
    assert bool((out == 0).all())


@pytest.mark.parametrize("B,L", [(3, 4133), (2, 4096), (1, 1)])
def test_identity_plan_copies(B, L):
    """speed 100, no notch, no chunks, no noise rows: S_in = S_out = W = 1, w = 1, the delta filter"""
    from speech_anonymization_amd import augment
    plan = augment.make_plan(B, L, 100)
    assert (plan.S_in, plan.S_out, plan.W, plan.Lp) == (1, 1, 1, L)
    wav = _wav(B, L, [1.0] * B, 5).to(DEV)
    out = augment.apply_plan(wav, torch.ones(B, device=DEV), plan)
    print(f"identity B={B} L={L}: {int((out != wav).sum())} elements differ")
    assert torch.equal(out, wav)


def test_same_plan_same_bits_and_side_stream():
    from speech_anonymization_amd import augment
    wav, noise = _wav(3, 4133, LENS3, 31).to(DEV), torch.randn(3, 4133, device=DEV)
    lens = torch.tensor(LENS3, device=DEV)
    plan = augment.draw_plan(torch.Generator().manual_seed(3), torch.tensor(LENS3), 4133)
    a = augment.apply_plan(wav, lens, plan, noise)
    b = augment.apply_plan(wav, lens, plan, noise)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = augment.apply_plan(wav, lens, plan, noise)
    s.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------
# the two small kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(3, 4133), (2, 5), (4, 8192)])
def test_abs_sums(B, L):
    """ragged batch, rows that start off a 16-byte boundary, a row shorter than one vector; 2 * 2^-24 relative"""
    from speech_anonymization_amd import ops
    wav = _wav(B, L, [1.0, 0.61, 0.33, 0.8][:B], 41)
    noise = torch.randn(B, L, generator=torch.Generator().manual_seed(42))
    got = ops.wav_abs_sums(wav.to(DEV), noise.to(DEV)).cpu()
    want = torch.stack([wav.double().abs().sum(1), noise.double().abs().sum(1)])
    rel = float(((got - want).abs() / want).max())
    print(f"abs sums B={B} L={L}: rel {rel:.3e}")
    assert got.dtype == torch.float64 and rel <= 2 * EPS
    only = ops.wav_abs_sums(wav.to(DEV)).cpu()
    assert torch.equal(only[0], got[0])


def test_noise_scales():
    from speech_anonymization_amd import ops
    B, L = 5, 4133
    lens = torch.tensor([1.0, 0.61, 0.33, 0.9, 0.5])
    wav = _wav(B, L, lens.tolist(), 51)
    noise = torch.randn(B, L, generator=torch.Generator().manual_seed(52))
    snr = torch.tensor([0.0, 15.0, 3.3, 7.7, 11.1])
    sums = torch.stack([wav.double().abs().sum(1), noise.double().abs().sum(1)])
    got = ops.noise_scales(sums.to(DEV), lens.to(DEV), snr.to(DEV), L).cpu()
    want = reference_scales(wav, noise, lens, snr)
    rel = float(((got.double() - want).abs() / want.abs()).max())
    print(f"noise scales: rel {rel:.3e}")
    assert got.dtype == torch.float32 and got.shape == (B, 2) and rel <= 2 * EPS


def test_refusals():
    from speech_anonymization_amd import augment, ops
    from speech_anonymization_amd._lib import SaHipError
    wav = torch.randn(2, 64)
    plan = augment.make_plan(2, 64, 100)
    words = plan.words().to(DEV)
    args = (2, 64, 1, 1, 1, 0, 0)
    with pytest.raises(SaHipError, match="GPU tensors"):
        ops.wav_augment(wav, None, None, words, *args)
    with pytest.raises(SaHipError, match="float32"):
        ops.wav_augment(wav.double().to(DEV), None, None, words, *args)
    with pytest.raises(SaHipError, match="contiguous"):
        ops.wav_augment(torch.randn(64, 2, device=DEV).t(), None, None, words, *args)
    with pytest.raises(SaHipError, match="rows"):
        ops.wav_augment(wav.to(DEV), None, None, words, 3, 64, 1, 1, 1, 0, 0)
    with pytest.raises(SaHipError, match="words"):
        ops.wav_augment(wav.to(DEV), None, None, words[:50], *args)
    with pytest.raises(SaHipError, match="GPU tensors"):
        ops.wav_augment(wav.to(DEV), wav, torch.ones(2, 2, device=DEV), words, 4, 64, 1, 1, 1, 0, 0)
    with pytest.raises(SaHipError, match="GPU tensors"):
        ops.wav_abs_sums(wav)
    with pytest.raises(SaHipError, match="float32"):
        ops.wav_abs_sums(wav.half().to(DEV))
    with pytest.raises(SaHipError, match="float64"):
        ops.noise_scales(torch.ones(2, 2, device=DEV), torch.ones(2, device=DEV), torch.ones(2, device=DEV), 64)
    with pytest.raises(SaHipError, match="needs the noise"):
        augment.apply_plan(wav.to(DEV), torch.ones(2, device=DEV), augment.make_plan(2, 64, 100, snr=[1.0, 2.0]))
    with pytest.raises(SaHipError, match="drawn for"):
        augment.apply_plan(torch.randn(2, 65, device=DEV), torch.ones(2, device=DEV), plan)
    with pytest.raises(SaHipError, match="code -22"):        # a 2:1 ratio does not fit the staging buffer: -EINVAL
        ops.wav_augment(wav.to(DEV), None, None, torch.zeros(4096, dtype=torch.int32, device=DEV), 2, 32, 2, 1, 13, -6, 6)
    with pytest.raises(SaHipError, match="GPU only"):
        augment.TrainAugment()(wav, torch.ones(2))


# ---------------------------------------------------------------------------------------------------
# the module and the recipe
# ---------------------------------------------------------------------------------------------------
class _Counting:
    """the loaded library with every sa_* call counted"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("sa_"):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_train_augment_end_to_end(monkeypatch):
    """[2 B, L'], lengths repeated, three launches of this library (constants are cached before counting), the
    noise drawn by the module's device generator: the same (seed, epoch) gives the same bits, another epoch not"""
    from speech_anonymization_amd import _lib, augment
    B, L = 4, 8000
    aug = augment.TrainAugment(seed=7)
    wav, lens = _wav(B, L, (1.0, 0.9, 0.8, 0.7), 61).to(DEV), torch.tensor([1.0, 0.9, 0.8, 0.7])
    augment.tile(), augment.max_chunks()
    aug.reseed(2)
    first, _, _ = aug(wav, lens.to(DEV), host_lens=lens)
    counting = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counting)
    aug.reseed(2)
    out, lens2, repeat = aug(wav, lens.to(DEV), host_lens=lens)
    monkeypatch.undo()
    plan = aug.last_plan
    print("launches:", counting.calls, "speed", plan.speed, "Lp", plan.Lp)
    assert counting.calls == ["sa_wav_abs_sums", "sa_noise_scales", "sa_wav_augment"]
    assert repeat == 2 and out.shape == (2 * B, plan.Lp)
    assert plan.Lp == augment.resampled_length(L, 16000, 160 * plan.speed)
    assert torch.equal(lens2.cpu(), torch.cat([lens, lens]))
    assert torch.equal(out, first)
    aug.reseed(3)
    other, _, _ = aug(wav, lens.to(DEV), host_lens=lens)
    assert other.shape != out.shape or not torch.equal(other, out)
    assert bool(torch.isfinite(out).all())


def _brain(tmp_path, augment_on):
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    with open(os.path.join(ROOT, "speechbrain_configs", "gender_classifier.yaml")) as f:
        st = load_hyperpyyaml(f, {"output_folder": str(tmp_path), "augment": augment_on, "batch_size": 4})
    hp = dict(st, **gender.build(st))
    b = gender.GenderBrain(modules=hp["modules"], opt_class=hp["opt_class"], hparams=hp, run_opts={"device": DEV})
    b.on_fit_start()
    return b


def test_fit_batch_with_augmentation(tmp_path):
    """one GenderBrain.fit_batch at B = 4, L = 8000 with augmentation on: a finite loss over 8 rows, all 30
    gradients filled; VALID-stage features bit-equal to those of a brain built without augmentation"""
    from speech_anonymization_amd.brain import Batch, Stage
    on, off = _brain(tmp_path / "on", True), _brain(tmp_path / "off", False)
    assert "augmentation" in on.modules and "augmentation" not in off.modules
    wav, lens = _wav(4, 8000, (1.0, 0.9, 0.8, 0.7), 71), torch.tensor([1.0, 0.9, 0.8, 0.7])
    batch = Batch(wav, lens, torch.tensor([0, 1, 1, 0]))
    for b in (on, off):
        b.modules.train()                                   # (two fresh normalisers: the same update in both)
    with torch.no_grad():
        fa = on.prepare_features(wav.to(DEV), lens.to(DEV), Stage.VALID)
        fb = off.prepare_features(wav.to(DEV), lens.to(DEV), Stage.VALID)
    assert torch.equal(fa, fb)
    on.on_stage_start(Stage.TRAIN, 1)
    on.modules.train()
    on.step = 1
    out = on.compute_forward(batch, Stage.TRAIN)
    assert out.shape == (8, 1, 2) and on._aug[1] == 2
    loss = on.compute_objectives(out, batch, Stage.TRAIN)
    loss.backward()
    params = list(on.modules.parameters())
    filled = sum(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
                 for p in params)
    print(f"loss {float(loss):.4f}, {filled} of {len(params)} gradients filled")
    assert bool(torch.isfinite(loss)) and len(params) == 30 and filled == 30
    on.optimizer.zero_grad()
    assert bool(torch.isfinite(on.fit_batch(batch)))


def test_recipe_learns_with_augmentation(tmp_path):
    """gender_classifier_train.py --synthetic 96 --number_of_epochs 4 --augment true in a fresh process within
    60 s of wall time.  Bar: the CPU rehearsal of the same data, seed, plan stream and budget
    (tools/gender_augment_cpu_rehearsal.py) reaches E_CPU; the GPU run must reach E_CPU + 0.1.  The best
    checkpoint loads through gender.load_external_classifier."""
    from speech_anonymization_amd import gender
    out = tmp_path / "gender_aug"
    cmd = [sys.executable, os.path.join(ROOT, "gender_classifier_train.py"),
           os.path.join(ROOT, "speechbrain_configs", "gender_classifier.yaml"), "--device", DEV,
           "--output_folder", str(out), "--synthetic", "96", "--number_of_epochs", "4", "--batch_size", "16",
           "--augment", "true"]
    t0 = time.monotonic()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    wall = time.monotonic() - t0
    print(r.stdout[-3000:], r.stderr[-3000:], f"\nrecipe wall time {wall:.1f} s")
    assert r.returncode == 0
    assert "waveform augmentation on" in r.stdout and "white" in r.stdout and "not part of this build" not in r.stdout
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(f"test error {res['test_error']} (CPU rehearsal {E_CPU}, bar {E_CPU + E_MARGIN}); wall {wall:.1f} s")
    assert wall <= 60.0, wall
    clf = gender.load_external_classifier(res["best_checkpoint"])
    assert not clf.training
    assert res["test_error"] <= E_CPU + E_MARGIN, res
