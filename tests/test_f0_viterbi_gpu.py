"""GPU checks of the Viterbi F0 tracker (csrc/sa_f0track.hip; ops.f0_candidates, ops.f0_viterbi,
pitchnorm.f0_track) against the restatement tests/f0v_ref.py.

Everything after d' is integer arithmetic, so the restatement is fed the GPU's OWN d' and candidates, paths and f0 are
compared for EQUALITY: cand_tau, cand_q and path exactly, f0 bit for bit (the refinement is a handful of fp64
operations each rounded correctly, a - 2 c + e with an exact product, so the device and numpy agree).  The scenario
claims are the ones tests/test_f0_viterbi_cpu.py makes of the restatement; tools/f0_viterbi_delta.py shows that no
decoded path of theirs moves when d' is rescaled by section 15's epsilon, which is what lets the fp32 d' of the GPU
stand in for the rounded fp64 one."""
import numpy as np
import pytest
import torch

from tests import f0v_ref as R

DEV = "cuda:0"
gpu = pytest.mark.gpu
LENS = (1.0, 1.0, 0.6, 1.0, 1.0, 1.0)


def _ops():
    from speech_anonymization_amd import ops
    return ops


class _Case:
    """the six scenario rows at a width N: the GPU's d', YIN track and candidates, and the restatement's candidates
    of that d' -- computed once and shared"""

    def __init__(self, wav):
        ops = _ops()
        self.wav = wav.to(DEV).contiguous()
        self.N = wav.shape[1]
        self.f0_y, self.dp = ops.yin_f0(self.wav, 0.15, return_dprime=True)
        self.tau, self.q = ops.f0_candidates(self.dp)
        self.dp_h = self.dp.cpu().numpy()
        self.tau_ref, self.q_ref = R.candidates(self.dp_h)


@pytest.fixture(scope="module")
def cases():
    rows = R.scenario_rows()
    return _Case(rows), _Case(rows[:, 1000:1500])


@gpu
def test_candidates_match_the_restatement_on_the_gpu_s_own_dprime(cases):
    for case, T in zip(cases, (R.T_CASE, 4)):
        assert tuple(case.tau.shape) == tuple(case.q.shape) == (6, T, R.K) and case.tau.dtype == torch.int32
        assert np.array_equal(case.tau.cpu().numpy(), case.tau_ref)
        assert np.array_equal(case.q.cpu().numpy(), case.q_ref)
    full = cases[0]
    assert int((full.tau_ref >= 0).sum(-1).max()) == R.K and not (full.tau_ref[5] >= 0).any()
    assert int((full.tau_ref[0] >= 0).sum(-1).min()) < R.K                  # full and partly filled frames both occur


@gpu
def test_decode_on_audio_is_the_restatement_s_path_and_bits(cases):
    ops = _ops()
    LOG = R.log_table()
    lens = torch.tensor(LENS, dtype=torch.float32, device=DEV)
    for case in cases:
        T = case.dp.shape[1]
        f0, path = ops.f0_viterbi(case.dp, case.tau, case.q, lens, case.N, return_path=True,
                                  log_q=torch.from_numpy(LOG).to(DEV))
        want = R.decode(case.tau_ref, case.q_ref, LENS, case.N, LOG)
        assert path.dtype == torch.int32 and np.array_equal(path.cpu().numpy(), want)
        want_f0 = R.refine(case.dp_h, R.lags_of(case.tau_ref, want))
        assert torch.equal(f0.cpu(), torch.from_numpy(want_f0))
        F = R.frames_counted(LENS, case.N, T)
        assert F[0] == T
        if T == R.T_CASE:
            assert F[2] == int(round(0.6 * case.N)) // 160 + 1 < T
            assert bool((f0[2, F[2]:] == 0).all()) and bool((path[2, F[2]:] == -1).all())
            assert bool((path[2, 2:F[2]] >= 0).all()) and bool((f0[2, 2:F[2]] > 0).all())
        f0_cached = ops.f0_viterbi(case.dp, case.tau, case.q, lens, case.N)   # the cached table is the same table
        assert torch.equal(f0_cached, f0)


@gpu
def test_decode_across_chunks_on_random_integer_candidates():
    ops = _ops()
    from speech_anonymization_amd import _lib
    chunk = _lib.load().sa_f0v_dim(3)
    B, T = 3, 3 * chunk + 5
    N = 160 * (T - 1)
    tau, q = R.random_candidates(B, T, seed=21)
    assert not (tau[:, T // 2] >= 0).any() and bool((tau < 0).any(-1).mean() > 0.5)
    g = torch.Generator().manual_seed(4)
    dp = torch.rand(B, T, 267, generator=g).to(DEV)
    lens_h = (1.0, 1.0, (2.0 * chunk + 0.5) / (T - 1))                       # the last row ends inside chunk 2
    lens = torch.tensor(lens_h, dtype=torch.float32, device=DEV)
    tau_d, q_d = torch.from_numpy(tau).to(DEV), torch.from_numpy(q).to(DEV)
    F = R.frames_counted(lens_h, N, T)
    assert F[:2] == [T, T] and 2 * chunk < F[2] < 3 * chunk
    seen = []
    for costs in (R.DEFAULTS, R.ZERO_TRANSITIONS):
        f0, path = ops.f0_viterbi(dp, tau_d, q_d, lens, N, return_path=True, **costs)
        want = R.decode(tau, q, lens_h, N, **costs)
        assert np.array_equal(path.cpu().numpy(), want)
        assert torch.equal(f0.cpu(), torch.from_numpy(R.refine(dp.cpu().numpy(), R.lags_of(tau, want))))
        assert bool((path[2, F[2]:] == -1).all()) and bool((f0[2, F[2]:] == 0).all())
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])                               # the transition weights matter here
    assert (seen[0] >= 0).any() and (seen[0] == -1).any() and (seen[0] > 0).any()


@gpu
def test_scenario_claims_on_f0_track(cases):
    from speech_anonymization_amd import pitchnorm
    wav = cases[0].wav
    f0_v = pitchnorm.f0_track(wav, method="viterbi")
    f0_y = pitchnorm.f0_track(wav, method="yin")
    assert tuple(f0_v.shape) == (6, R.T_CASE) and f0_v.dtype == torch.float32
    R.check_scenarios(f0_v.cpu().numpy(), f0_y.cpu().numpy(), report=print)


@gpu
def test_same_bits_as_yin_where_both_pick_the_same_lag(cases):
    from speech_anonymization_amd import pitchnorm
    ops = _ops()
    case = cases[0]
    lens = torch.ones(6, dtype=torch.float32, device=DEV)
    f0_v, path = ops.f0_viterbi(case.dp, case.tau, case.q, lens, case.N, return_path=True)
    lag_v = R.lags_of(case.tau_ref, path.cpu().numpy())
    _, lag_y = R.yin_f0(case.dp_h)                                             # first-dip YIN's lag on the same d'
    same = torch.from_numpy((lag_v == lag_y) & (lag_y > 0)).to(DEV)
    assert int(same.sum()) >= 120 and int((~same).sum()) >= 8
    assert torch.equal(f0_v[same], case.f0_y[same])
    assert torch.equal(pitchnorm.f0_track(case.wav), ops.yin_f0(case.wav, 0.15))
    assert torch.equal(pitchnorm.f0_track(case.wav), case.f0_y)
    assert torch.equal(pitchnorm.f0_track(case.wav, method="viterbi"), f0_v)


@gpu
def test_through_the_class_on_the_weak_fundamental_row(cases):
    from speech_anonymization_amd import pitchnorm
    wav, lens = cases[0].wav[:1].contiguous(), torch.ones(1)
    pn = pitchnorm.PitchNormalizer(170, phase="vocoder", f0_method="viterbi")
    out = pn(wav, lens)
    assert tuple(out.shape) == tuple(wav.shape) and bool(torch.isfinite(out).all())
    ratio, mean, voiced = (float(v[0]) for v in pn.last)
    print(f"viterbi: mean {mean:.3f} Hz over {voiced:.0f} frames, ratio {ratio:.5f}")
    assert abs(mean - 100.0) <= 1.0
    assert abs(ratio - 170.0 / mean) <= 4 * 2.0 ** -24 * ratio              # (formed in fp64 from the unrounded mean)
    py = pitchnorm.PitchNormalizer(170, phase="vocoder", f0_method="yin")
    py(wav, lens)
    print(f"yin: mean {float(py.last[1][0]):.3f} Hz")
    assert float(py.last[1][0]) > 110.0
    pc = pitchnorm.PitchNormalizer(170, phase="vocoder", f0_method="viterbi", contour_scale=1.0)   # shift_contour
    pc(wav, lens)
    assert abs(float(pc.last[1][0]) - 100.0) <= 1.0


@gpu
def test_two_runs_are_bit_identical_and_bad_tensors_are_refused(cases):
    from speech_anonymization_amd import _lib, pitchnorm
    ops = _ops()
    case = cases[0]
    lens = torch.tensor(LENS, dtype=torch.float32, device=DEV)
    tau2, q2 = ops.f0_candidates(case.dp)
    assert torch.equal(tau2, case.tau) and torch.equal(q2, case.q)
    a = ops.f0_viterbi(case.dp, case.tau, case.q, lens, case.N, return_path=True)
    b = ops.f0_viterbi(case.dp, case.tau, case.q, lens, case.N, return_path=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(pitchnorm.f0_track(case.wav, method="viterbi", lens=lens),
                       pitchnorm.f0_track(case.wav, method="viterbi", lens=lens))
    assert torch.equal(pitchnorm.f0_track(case.wav, method="viterbi", lens=lens), a[0])
    Err = _lib.SaHipError
    with pytest.raises(Err, match="GPU tensors"):
        ops.f0_candidates(case.dp.cpu())
    with pytest.raises(Err, match="contiguous"):
        ops.f0_candidates(case.dp.transpose(0, 1))
    with pytest.raises(Err, match="float32"):
        ops.f0_candidates(case.dp.double())
    with pytest.raises(Err, match="267"):
        ops.f0_candidates(case.dp[..., :266].contiguous())
    with pytest.raises(Err, match="GPU tensors"):
        ops.f0_viterbi(case.dp, case.tau.cpu(), case.q, lens, case.N)
    with pytest.raises(Err, match="contiguous"):
        ops.f0_viterbi(case.dp, case.tau, case.q.transpose(0, 1).contiguous().transpose(0, 1), lens, case.N)
    with pytest.raises(Err, match="int32"):
        ops.f0_viterbi(case.dp, case.tau.long(), case.q, lens, case.N)
    with pytest.raises(Err, match="float32"):
        ops.f0_viterbi(case.dp, case.tau, case.q, lens.double(), case.N)
    with pytest.raises(Err, match="shape"):
        ops.f0_viterbi(case.dp, case.tau, case.q, lens[:5].contiguous(), case.N)
    with pytest.raises(Err, match="int32"):
        ops.f0_viterbi(case.dp, case.tau, case.q, lens, case.N, log_q=ops.f0v_log_table(DEV).long())
    with pytest.raises(Err, match="costs in"):
        ops.f0_viterbi(case.dp, case.tau, case.q, lens, case.N, jump_cost=float("nan"))
    with pytest.raises(Err, match="N = 0"):
        ops.f0_viterbi(case.dp, case.tau, case.q, lens, 0)
