"""The TD-PSOLA kernels (csrc/sa_psola.hip) against the restatement of tests/psola_ref.py: marks and
plan entry for entry, the overlap-add within the bar tools/psola_delta.py measured on the restatement's own fp32
variant (profiles/psola_delta.json), then PitchNormalizer(psola=True), anonymize.py and the recipe.

The kernel cases (psola_ref.kernel_cases): B = 5, N = 4000 (T = 26) -- a 110 Hz voice in noise at ratio 1; a 200 -> 260
Hz glide with frames 9..13 unvoiced at 1.417; noise with no voiced frame under a ramp of the ratio over its whole range;
a voiced row of 700 valid samples at 0.5; a row of none under ratios outside the range -- then B = 1, N = 159 (T = 1),
and a row of equal samples, where every argmax is a tie."""
import importlib.util
import json
import math
import os

import pytest
import torch

from tests import anon_cli
from tests import contour_ref as CR
from tests import formant_ref as F
from tests import psola_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
gpu = pytest.mark.gpu
with open(os.path.join(ROOT, "profiles", "psola_delta.json")) as _f:
    DELTA = json.load(_f)
CASES = ("batch", "short", "tie")
EINVAL = -22


@pytest.fixture(scope="module")
def cases():
    """name -> (the inputs on the CPU, the restatement's tables per row, its fp64 output): computed once"""
    out = {}
    for name, inp in R.kernel_cases().items():
        rows = R.tables(*inp)
        out[name] = (inp, rows, R.psola(*inp, rows=rows))
    return out


def _dev(inp):
    return tuple(t.to(DEV).contiguous() for t in inp)


def _run(inp):
    """-> (marks, count, syn_pos, syn_src, syn_count, out) of the three kernels"""
    from speech_anonymization_amd import ops
    wav, f0, rho_q, nv = _dev(inp)
    marks, count = ops.psola_marks(wav, f0, nv)
    pos, src, jc = ops.psola_plan(marks, count, f0, rho_q, nv, N=wav.shape[1])
    return marks, count, pos, src, jc, ops.psola_ola(wav, marks, count, pos, src, jc, nv)


@gpu
@pytest.mark.parametrize("name", CASES)
def test_marks_and_plan_equal_the_restatement(cases, name):
    inp, rows, _ = cases[name]
    marks, count, pos, src, jc, _ = (t.cpu() for t in _run(inp))
    N = inp[0].shape[1]
    assert marks.shape[1] == R.mcap(N) and pos.shape[1] == src.shape[1] == R.jcap(N)
    for b, (mk, p, s) in enumerate(rows):
        assert int(count[b]) == len(mk) and int(jc[b]) == len(p), (b, int(count[b]), len(mk), int(jc[b]), len(p))
        assert marks[b, :len(mk)].tolist() == mk, b
        assert pos[b, :len(p)].tolist() == p and src[b, :len(p)].tolist() == s, b
    if name == "batch":                                          # the cases are what the docstring says they are
        assert [len(r[0]) > 1 for r in rows] == [True, True, True, True, False] and len(rows[3][1]) >= 2
        assert rows[2][0] == list(range(0, N, 80))


@gpu
def test_marks_order_nan_signed_zeros_denormals_and_infinities_as_the_restatement_does():
    """the argmax is by value with >, a NaN as -inf and ties to the smallest index: rows whose windows hold NaNs only,
    +0 and -0 only (equal: the first wins), denormals, and infinities of both signs"""
    from speech_anonymization_amd import ops
    g = torch.Generator().manual_seed(2428)
    N, T = 2000, 13
    base = 0.1 * torch.randn(N, generator=g)
    nan = base.clone()
    nan[::3] = float("nan")
    nan[300:700] = float("nan")
    zeros = torch.zeros(N)
    zeros[torch.rand(N, generator=g) < 0.5] = -0.0
    tiny = torch.where(torch.rand(N, generator=g) < 0.5, 1e-42, -1e-42) * torch.randint(1, 9, (N,), generator=g)
    tiny[::7] = 0.0
    inf = base.clone()
    inf[100::150] = float("inf")
    inf[40::150] = float("-inf")
    inf[1000:1400] = float("-inf")
    wav = torch.stack([nan, zeros, tiny, inf]).float()
    f0 = torch.tensor([150.0, 90.0, 333.0, 61.0])[:, None].expand(4, T).contiguous()
    nv = torch.full((4,), N, dtype=torch.int32)
    marks, count = (t.cpu() for t in ops.psola_marks(wav.to(DEV), f0.to(DEV), nv.to(DEV)))
    for b in range(4):
        mk = R.marks(wav[b].numpy(), f0[b].numpy(), N)
        assert int(count[b]) == len(mk) > 5 and marks[b, :len(mk)].tolist() == mk, b


@gpu
def test_first_mark_is_searched_over_the_whole_first_period():
    """the first window is [0, per[0] - 1], up to 266 samples and so more than the 133 of every later one: voices of 60
    to 75 Hz whose largest sample of that window lies at index 192 or beyond, up to its last sample"""
    from speech_anonymization_amd import ops
    g = torch.Generator().manual_seed(2429)
    N, T = 2000, 13
    hz, peak = (60.0, 61.0, 66.0, 70.0, 75.0), (265, 200, 241, 228, 192)       # periods 266 (clamped), 262, 242, 229, 213
    wav = 0.1 * torch.randn(len(hz), N, generator=g)
    for b, i in enumerate(peak):
        wav[b, i] = 5.0
        wav[b, i + 1] = 7.0 if b == 0 else wav[b, i + 1]         # (row 0: a larger sample one past the window)
    f0 = torch.tensor(hz)[:, None].expand(len(hz), T).contiguous()
    nv = torch.full((len(hz),), N, dtype=torch.int32)
    marks, count = (t.cpu() for t in ops.psola_marks(wav.to(DEV), f0.to(DEV), nv.to(DEV)))
    for b, i in enumerate(peak):
        mk = R.marks(wav[b].numpy(), f0[b].numpy(), N)
        assert mk[0] == i and int(R.periods(f0[b].numpy(), N)[0]) > i >= 192, (b, mk[0])
        assert int(count[b]) == len(mk) > 5 and marks[b, :len(mk)].tolist() == mk, b


@gpu
@pytest.mark.parametrize("name", CASES)
def test_overlap_add_against_fp64(cases, name):
    inp, _, ref = cases[name]
    out = _run(inp)[5].cpu().double()
    scale = inp[0].abs().amax(1).double().clamp(min=1e-30)[:, None]
    err = ((out - ref).abs() / scale)
    print(name, "worst |out - ref| / max|wav|", float(err.max()), "bar", DELTA["ola_bar"])
    assert torch.isfinite(out).all() and float(err.max()) <= DELTA["ola_bar"]
    live = torch.arange(out.shape[1])[None, :] < inp[3][:, None]
    assert float((out * ~live).abs().max()) == 0.0
    assert ops_psola(inp).equal(_run(inp)[5])                    # ops.psola is the three launches


def ops_psola(inp):
    from speech_anonymization_amd import ops
    return ops.psola(*_dev(inp))


@gpu
@pytest.mark.parametrize("name", CASES)
def test_identity_at_ratio_one(cases, name):
    wav, f0, rho_q, nv = cases[name][0]
    out = ops_psola((wav, f0, torch.full_like(rho_q, R.RHO_ONE), nv)).cpu()
    live = torch.arange(wav.shape[1])[None, :] < nv[:, None]
    bound = 1e-6 * wav.abs().amax(1)[:, None]
    worst = float((((out - wav).abs() - bound) * live).max())
    print(name, "worst |out - wav| / max|wav|", float(((out - wav).abs() * live / wav.abs().amax(1)[:, None]).max()))
    assert worst <= 0.0 and float((out * ~live).abs().max()) == 0.0


@gpu
def test_two_runs_and_a_row_alone_give_the_same_bits(cases):
    inp = cases["batch"][0]
    first, again = _run(inp), _run(inp)
    assert all(torch.equal(first[i], again[i]) for i in (1, 4, 5))
    for b in range(inp[0].shape[0]):                             # (entries past a row's count mean nothing)
        for alone in (tuple(t[b:b + 1] for t in again), _run(tuple(t[b:b + 1] for t in inp))):
            _same_row(alone, first, b)


def _same_row(alone, first, b):
    nm, nj = int(alone[1][0]), int(alone[4][0])
    assert nm == int(first[1][b]) and nj == int(first[4][b])
    assert torch.equal(alone[0][0, :nm], first[0][b, :nm]) and torch.equal(alone[2][0, :nj], first[2][b, :nj])
    assert torch.equal(alone[3][0, :nj], first[3][b, :nj]) and torch.equal(alone[5][0], first[5][b])


@gpu
def test_refused_calls_leave_the_outputs_untouched(cases):
    from speech_anonymization_amd import _lib, ops
    lib = _lib.load()
    wav, f0, rho_q, nv = _dev(cases["batch"][0])
    B, N, T = 5, 4000, 26
    marks, count, pos, src, jc, _ = _run(cases["batch"][0])
    ws = torch.empty(lib.sa_psola_workspace_bytes(B, N) // 8, dtype=torch.int64, device=DEV)
    assert lib.sa_psola_workspace_bytes(B, N) == 8 * B * R.mcap(N)
    p = _lib.ptr

    def poison(*shapes):
        return [torch.full(s, -77, dtype=torch.int32, device=DEV) for s in shapes]

    def run_marks(a):
        o = poison((B, R.mcap(N)), (B,))
        args = dict(wav=p(wav), f0=p(f0), nv=p(nv), B=B, N=N, T=T, marks=p(o[0]), count=p(o[1]))
        args.update(a)
        return lib.sa_psola_marks(args["wav"], args["f0"], args["nv"], args["B"], args["N"], args["T"], args["marks"],
                                  args["count"], _lib.stream()), o

    def run_plan(a):
        o = poison((B, R.jcap(N)), (B, R.jcap(N)), (B,))
        args = dict(marks=p(marks), count=p(count), f0=p(f0), rho=p(rho_q), nv=p(nv), B=B, N=N, T=T, ws=p(ws),
                    pos=p(o[0]), src=p(o[1]), jc=p(o[2]))
        args.update(a)
        return lib.sa_psola_plan(args["marks"], args["count"], args["f0"], args["rho"], args["nv"], args["B"],
                                 args["N"], args["T"], args["ws"], args["pos"], args["src"], args["jc"],
                                 _lib.stream()), o

    def run_ola(a):
        o = [torch.full((B, N), -77.0, device=DEV)]
        args = dict(wav=p(wav), marks=p(marks), count=p(count), pos=p(pos), src=p(src), jc=p(jc), nv=p(nv), B=B, N=N,
                    out=p(o[0]))
        args.update(a)
        return lib.sa_psola_ola(args["wav"], args["marks"], args["count"], args["pos"], args["src"], args["jc"],
                                args["nv"], args["B"], args["N"], args["out"], _lib.stream()), o

    sizes = [{"B": 0}, {"B": 65536}, {"N": 0}, {"N": (1 << 24) + 1}]
    frames = [{"T": T - 1}, {"T": T + 1}, {"T": 0}]              # N = 4000 is a multiple of the hop: 26 frames only
    for run, keys, extra in ((run_marks, ("wav", "f0", "nv", "marks", "count"), frames),
                             (run_plan, ("marks", "count", "f0", "rho", "nv", "ws", "pos", "src", "jc"), frames),
                             (run_ola, ("wav", "marks", "count", "pos", "src", "jc", "nv", "out"), [])):
        for bad in [{k: None} for k in keys] + sizes + extra:
            rc, outs = run(bad)
            torch.cuda.synchronize()
            assert rc == EINVAL, (run.__name__, bad, rc)
            assert all(bool((o == -77).all()) for o in outs), (run.__name__, bad)
        rc, outs = run({})
        assert rc == 0 and not any(bool((o == -77).all()) for o in outs)
    # the padded width's frame count is the other T the entry points take: N = 159 -> 1 or 2 frames
    one, nv1 = torch.zeros(1, 159, device=DEV), torch.tensor([159], dtype=torch.int32, device=DEV)
    for T1, rc in ((1, 0), (2, 0), (3, EINVAL)):
        o, f01 = poison((1, R.mcap(159)), (1,)), torch.zeros(1, T1, device=DEV)
        assert lib.sa_psola_marks(p(one), p(f01), p(nv1), 1, 159, T1, p(o[0]), p(o[1]), _lib.stream()) == rc
        torch.cuda.synchronize()
        assert o[1].tolist() == ([2] if rc == 0 else [-77])       # unvoiced: marks at 0 and 80
    assert [lib.sa_psola_dim(i) for i in range(9)] == [80, 40, 266, 30, 332, 256, 30, 15, EINVAL]
    assert lib.sa_psola_dim(-1) == EINVAL and (ops.PSOLA_MDIV, ops.PSOLA_JDIV) == (30, 15)
    for B1, N1 in ((0, 100), (65536, 100), (1, 0), (1, (1 << 24) + 1)):
        assert lib.sa_psola_workspace_bytes(B1, N1) == EINVAL


@gpu
def test_wrappers_refuse_what_the_kernels_do_not_take(cases):
    from speech_anonymization_amd import _lib, ops
    inp = cases["batch"][0]
    wav, f0, rho_q, nv = _dev(inp)
    marks, count = ops.psola_marks(wav, f0, nv)
    bad = [lambda: ops.psola_marks(inp[0], f0, nv), lambda: ops.psola_marks(wav, inp[1], nv),
           lambda: ops.psola_marks(wav.t().contiguous().t(), f0, nv), lambda: ops.psola_marks(wav.double(), f0, nv),
           lambda: ops.psola_marks(wav, f0, nv.long()), lambda: ops.psola_marks(wav, f0[:, :25].contiguous(), nv),
           lambda: ops.psola_marks(wav, f0[:4], nv), lambda: ops.psola_plan(marks.cpu(), count, f0, rho_q, nv, N=4000),
           lambda: ops.psola_plan(marks, count, f0, rho_q.float(), nv, N=4000),
           lambda: ops.psola_plan(marks, count, f0, rho_q[:, ::2], nv, N=4000),
           lambda: ops.psola_plan(marks, count, f0, rho_q, nv, N=4030),
           lambda: ops.psola_plan(marks[:, :-1].contiguous(), count, f0, rho_q, nv, N=4000),
           lambda: ops.psola(wav, f0, rho_q.long(), nv), lambda: ops.psola(wav, f0, rho_q, nv[:4]),
           lambda: ops.psola(wav[0], f0, rho_q, nv)]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.SaHipError):
            call()
            pytest.fail(f"call {i} was taken")


# ---- the class ---------------------------------------------------------------------------------------
def _edge_mean(f0, N):
    return R.voiced_mean_f0(f0.cpu(), torch.ones(f0.shape[0]), N)


@gpu
def test_pitch_normalizer_moves_the_pitch_and_keeps_the_envelope():
    from speech_anonymization_amd import ops, pitchnorm
    wav = F.resonance_rows().to(DEV)
    lens = torch.ones(3, device=DEV)
    pn = pitchnorm.PitchNormalizer(DELTA["target_hz"], psola=True)
    out = pn(wav, lens)                                          # (warm-up: the library loads, the tables are made)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                      # a device-to-host copy raises from here on
    try:
        again = pn(wav, lens)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(out, again) and out.shape == wav.shape and out.dtype == torch.float32
    ratio = ops.pitch_ratio(ops.yin_f0(wav), lens, wav.shape[1], DELTA["target_hz"])
    assert all(torch.equal(a, b) for a, b in zip(pn.last, ratio))
    mean = _edge_mean(ops.yin_f0(out), wav.shape[1])
    peak_in, peak_out = F.envelope_peak(wav.cpu()), F.envelope_peak(out.cpu())
    print("mean F0", mean.tolist(), "peaks", peak_in.tolist(), "->", peak_out.tolist())
    assert float((mean - DELTA["target_hz"]).abs().max()) <= DELTA["f0_bar_hz"]
    assert float((peak_out - peak_in).abs().max()) <= DELTA["peak_bar_hz"]


@gpu
def test_pitch_normalizer_flattens_the_contour_at_scale_zero():
    from speech_anonymization_amd import ops, pitchnorm
    wav = CR.case_rows().to(DEV)
    lens = torch.ones(2, device=DEV)
    pn = pitchnorm.PitchNormalizer(DELTA["target_hz"], psola=True, contour_scale=0.0)
    out = pn(wav, lens)
    _, std_in, _ = CR.f0_stats(ops.yin_f0(wav).cpu(), lens.cpu(), wav.shape[1])
    mean, std, _ = CR.f0_stats(ops.yin_f0(out).cpu(), lens.cpu(), wav.shape[1])
    print("std", std_in.tolist(), "->", std.tolist(), "mean", mean.tolist(), "ratio", pn.last[0].tolist())
    assert float(std.max()) <= DELTA["contour_bar_hz"] < 0.5 * float(std_in.min())
    assert float((mean - DELTA["target_hz"]).abs().max()) <= DELTA["f0_bar_hz"]
    assert pn.last[0].shape == (2,) and pn.last[2].dtype == torch.int32
    with pytest.raises(pitchnorm.L.SaHipError, match="contour_scale needs 2 frames"):       # one frame: no contour
        pn(torch.zeros(1, 159, device=DEV), torch.ones(1, device=DEV))
    short = pitchnorm.PitchNormalizer(DELTA["target_hz"], psola=True)(wav[:, :159].contiguous(), lens)
    # (one frame, under min_voiced: ratio 1, the identity within its bar of 1e-6 max|wav|)
    assert float((short - wav[:, :159]).abs().max()) <= 1e-6 * float(wav[:, :159].abs().max())


# ---- the command line and the recipe -------------------------------------------------------------------
@gpu
def test_anonymize_writes_the_psola_waveforms(tmp_path, capsys):
    """--pitch_norm true --psola true --synthetic 4 --report_f0 true: the WAVs, "psola": true, "n_iter": null, and every
    utterance's f0_mean_hz within the F0 bar of the target"""
    from speech_anonymization_amd import data
    res = anon_cli.run(capsys, ["--device", DEV, "--out_dir", str(tmp_path), "--synthetic", "4", "--pitch_norm", "true",
                                "--psola", "true", "--report_f0", "true"])
    assert res["psola"] is True and res["n_iter"] is None and res["pitch_norm"] is True
    assert sorted(os.listdir(tmp_path)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    print([(u["ratio"], u["f0_mean_hz"], u["voiced_share"]) for u in res["utterances"]])
    for u in res["utterances"]:
        assert data.read_audio(os.path.join(tmp_path, u["id"] + ".wav")).numel() == u["samples"] > 0, u
    for u in res["utterances"]:
        assert abs(u["f0_mean_hz"] - res["pitch_target_hz"]) <= DELTA["f0_bar_hz"], u


@gpu
def test_anonymize_without_the_option_is_what_it_was(tmp_path):
    """two children: --pitch_norm true as it always ran, and the same with --psola false -- the same bytes in every
    file and the same JSON but for the key that was given; without the option the key is absent.  The parent commit
    cannot be run inside a test session, so this shows only that the key is inert on the code as it stands; that
    ``--pitch_norm true`` writes what the parent wrote rests on tools/anon_digest.py, whose digests of every existing
    mode were compared with the parent's on one GPU."""
    def child(name, extra):
        out = tmp_path / name
        res = anon_cli.run_child(["--device", DEV, "--out_dir", str(out), "--synthetic", "4", "--pitch_norm", "true",
                                  "--n_iter", "4", "--report_f0", "true"] + extra)
        files = {n: open(out / n, "rb").read() for n in sorted(os.listdir(out))}
        assert res.pop("out_dir") == str(out)
        return res, files

    plain, plain_files = child("plain", [])
    off, off_files = child("off", ["--psola", "false"])
    assert "psola" not in plain and plain["n_iter"] == 4 and off.pop("psola") is False
    assert json.dumps(plain) == json.dumps(off) and list(plain_files) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    assert plain_files == off_files


@gpu
def test_recipe_trains_one_epoch_with_psola(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("gender_classifier_train_pitch_norm",
                                                  os.path.join(ROOT, "gender_classifier_train_pitch_norm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main([os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml"), "--device", DEV,
              "--output_folder", str(tmp_path / "psola"), "--synthetic", "16", "--batch_size", "8",
              "--number_of_epochs", "1", "--psola", "true"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(res)
    assert math.isfinite(res["test_loss"]) and 0.0 <= res["test_error"] <= 1.0 and res["psola"] is True
    assert res["best_checkpoint"] and os.path.isdir(res["best_checkpoint"])
