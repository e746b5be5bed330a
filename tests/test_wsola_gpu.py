"""The WSOLA time-scale modification on the GPU (include/sa_hip.h carries the definition) against the
restatement tests/wsola_ref.py.

There is no error bar on the kernels: every entry of q, pos (up to count), count and n_out equals the restatement's,
and every element of out is equal in bits, no element left out.  The one measured bar is on what the transform is for:
the output's voiced-mean F0 stays at the input's within profiles/wsola_delta.json's ``f0_bar_hz``, twice the sum of what
the restatement itself moves it by and of the tracker's own distance from the generators' fundamentals (read, not typed
in; tools/wsola_delta.py measures it on the CPU)."""
import ctypes
import errno
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from speech_anonymization_amd import timescale
from tests import anon_cli
from tests import wsola_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
gpu = pytest.mark.gpu
H, ONE = R.H, R.ONE
POISON_I, POISON_Q = -77, 0x5A5A
with open(os.path.join(ROOT, "profiles", "wsola_delta.json")) as _f:
    DELTA = json.load(_f)

CASES = R.kernel_cases()
_reference = {}


def _ref(name):
    """the restatement of a case, computed once and shared"""
    if name not in _reference:
        _reference[name] = R.reference(CASES[name])
    return _reference[name]


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _kcap(Nout):
    return (Nout - 1) // H + 1


class Buffers:
    """the inputs of a case on the device and poisoned outputs: out NaN, the tables -77, the workspace 0x5a5a"""

    def __init__(self, case):
        from speech_anonymization_amd import ops
        wav, nv, tq, self.Nout = case
        self.B, self.N = wav.shape
        self.wav, self.nv, self.tq = _dev(wav, torch.float32), _dev(nv, torch.int32), _dev(tq, torch.int32)
        self.hann = ops.wsola_window(DEV)
        self.ws = ops.wsola_workspace(self.B, self.N, DEV).fill_(POISON_Q)
        self.out = torch.full((self.B, self.Nout), float("nan"), device=DEV)
        self.pos = torch.full((self.B, _kcap(self.Nout)), POISON_I, dtype=torch.int32, device=DEV)
        self.count, self.n_out = (torch.full((self.B,), POISON_I, dtype=torch.int32, device=DEV) for _ in range(2))

    def q(self):
        return self.ws[:self.B * self.N].view(self.B, self.N)

    def untouched(self):
        return bool(torch.isnan(self.out).all()) and all(bool((t == POISON_I).all()) for t in
                                                         (self.pos, self.count, self.n_out)) \
            and bool((self.ws == POISON_Q).all())


def _three(buf):
    """the three entry points in a row, through the library itself"""
    from speech_anonymization_amd import _lib
    lib, st = _lib.load(), _lib.stream()
    assert lib.sa_wsola_quant(_f(buf.wav), _f(buf.nv), buf.B, buf.N, _f(buf.ws), st) == 0
    assert lib.sa_wsola_search(_f(buf.ws), _f(buf.tq), _f(buf.nv), buf.B, buf.N, buf.Nout, _f(buf.pos), _f(buf.count),
                               _f(buf.n_out), st) == 0
    assert lib.sa_wsola_ola(_f(buf.wav), _f(buf.pos), _f(buf.count), _f(buf.tq), _f(buf.nv), _f(buf.hann), buf.B,
                            buf.N, buf.Nout, _f(buf.out), st) == 0
    torch.cuda.synchronize()
    return buf


def _one(buf):
    from speech_anonymization_amd import _lib
    assert _lib.load().sa_wsola(_f(buf.wav), _f(buf.tq), _f(buf.nv), _f(buf.hann), buf.B, buf.N, buf.Nout, _f(buf.ws),
                                _f(buf.out), _f(buf.pos), _f(buf.count), _f(buf.n_out), _lib.stream()) == 0
    torch.cuda.synchronize()
    return buf


def _assert_equals_restatement(buf, ref, what):
    q, pos = buf.q().cpu().numpy(), buf.pos.cpu().numpy()
    count, n_out = buf.count.cpu().tolist(), buf.n_out.cpu().tolist()
    out = buf.out.cpu().numpy()
    for b, (r_out, r_q, r_pos, r_K, r_n) in enumerate(ref):
        assert (count[b], n_out[b]) == (r_K, r_n), (what, b, count[b], n_out[b], r_K, r_n)
        bad = np.flatnonzero(q[b] != r_q)
        assert bad.size == 0, (what, b, "q", bad[:5], q[b][bad[:5]], r_q[bad[:5]])
        assert pos[b, :r_K].tolist() == r_pos, (what, b, "pos",
                                                [(k, int(pos[b, k]), r_pos[k]) for k in range(r_K)
                                                 if pos[b, k] != r_pos[k]][:5])
        assert (pos[b, r_K:] == POISON_I).all(), (what, b, "pos past count was written")
        bad = np.flatnonzero(out[b].view(np.uint32) != r_out.view(np.uint32))
        assert bad.size == 0, (what, b, "out", bad.size, bad[:5], out[b][bad[:5]], r_out[bad[:5]])


# ---------------------------------------------------------------------------------------------------
# the kernels against the restatement
# ---------------------------------------------------------------------------------------------------
@gpu
def test_dims_lengths_and_workspace():
    from speech_anonymization_amd import _lib, ops
    lib = _lib.load()
    assert [lib.sa_wsola_dim(i) for i in range(7)] == [160, 320, 160, 16383, 8192, 1024, 4096]
    assert lib.sa_wsola_dim(7) == lib.sa_wsola_dim(-1) == -errno.EINVAL
    assert (ops.WSOLA_H, ops.WSOLA_W, ops.WSOLA_D, ops.WSOLA_Q, ops.WSOLA_QTILE) == (160, 320, 160, 16383, 4096)
    for n in (0, 1, 159, 160, 4000, 4001, 1 << 24):
        for tq in (0, 1 << 15, ONE - 1, ONE, ONE + 1, 52429, 81920, 1 << 17, 1 << 20, -3):
            assert lib.sa_wsola_out_len(n, tq) == R.out_len(n, tq) == ops.wsola_out_len(n, tq), (n, tq)
    assert lib.sa_wsola_out_len(-1, ONE) == lib.sa_wsola_out_len((1 << 24) + 1, ONE) == -errno.EINVAL
    for B, N in ((1, 1), (5, 4000), (3, 4093), (3, 4094), (1, 159), (65535, 1 << 24), (32, 160000)):
        assert lib.sa_wsola_workspace_bytes(B, N) == ops.wsola_workspace_bytes(B, N), (B, N)
    for B, N in ((0, 100), (65536, 100), (1, 0), (1, (1 << 24) + 1), (-1, 5)):
        assert lib.sa_wsola_workspace_bytes(B, N) == -errno.EINVAL


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_restatement_in_every_entry_and_bit(name):
    from speech_anonymization_amd import ops
    ref = _ref(name)
    buf = _three(Buffers(CASES[name]))
    _assert_equals_restatement(buf, ref, name)
    one = _one(Buffers(CASES[name]))                         # sa_wsola: the same tables and the same bits
    _assert_equals_restatement(one, ref, name + " (one call)")
    # through ops: the three calls and the one
    q = ops.wsola_quant(buf.wav, buf.nv)
    pos, count, n_out = ops.wsola_search(q, buf.tq, buf.nv, buf.Nout)
    out = ops.wsola_ola(buf.wav, pos, count, buf.tq, buf.nv, buf.Nout)
    assert torch.equal(q, buf.q()) and torch.equal(count, buf.count) and torch.equal(n_out, buf.n_out)
    assert torch.equal(_bits(out), _bits(buf.out))
    out1, n_out1, pos1, count1 = ops.wsola(buf.wav, buf.tq, buf.nv, buf.Nout, return_pos=True)
    assert torch.equal(_bits(out1), _bits(out)) and torch.equal(n_out1, n_out) and torch.equal(count1, count)
    live = torch.arange(pos.shape[1], device=DEV)[None, :] < count[:, None]
    assert torch.equal(pos[live], pos1[live]) and torch.equal(pos[live], buf.pos[live])
    assert len(ops.wsola(buf.wav, buf.tq, buf.nv, buf.Nout)) == 2


@gpu
def test_tempo_one_returns_the_input_bit_for_bit():
    from speech_anonymization_amd import ops
    wav, nv, _, _ = R.edge_case()
    wd, nvd = _dev(wav, torch.float32), _dev(nv, torch.int32)
    out, n_out = ops.wsola(wd, torch.full((6,), ONE, dtype=torch.int32, device=DEV), nvd, wav.shape[1])
    assert n_out.cpu().tolist() == nv
    live = torch.arange(wav.shape[1], device=DEV)[None, :] < nvd[:, None]
    assert torch.equal(_bits(out)[live], _bits(wd)[live]) and not _bits(out)[~live].any()


@gpu
def test_two_runs_and_every_row_alone_give_the_same_bits():
    for name in ("batch", "odd", "long"):
        wav, nv, tq, Nout = CASES[name]
        first, second = _one(Buffers(CASES[name])), _one(Buffers(CASES[name]))
        assert torch.equal(_bits(first.out), _bits(second.out)) and torch.equal(first.pos, second.pos)
        assert torch.equal(first.q(), second.q())
        for b in range(wav.shape[0]):
            alone = _one(Buffers((wav[b:b + 1], nv[b:b + 1], tq[b:b + 1], Nout)))
            assert torch.equal(_bits(alone.out[0]), _bits(first.out[b])), (name, b)
            assert torch.equal(alone.pos[0], first.pos[b]) and torch.equal(alone.q()[0], first.q()[b]), (name, b)
            assert int(alone.count[0]) == int(first.count[b]) and int(alone.n_out[0]) == int(first.n_out[b])


@gpu
def test_tables_the_kernels_did_not_write_are_clamped():
    """sa_wsola_ola under a pos, a count, an n_valid and a tempo_q far outside their ranges: it reads inside the row
    (positions into [0, N], the count into [0, Kcap]) and writes all of out, nothing else"""
    from speech_anonymization_amd import _lib
    buf = Buffers(CASES["batch"])
    kc = _kcap(buf.Nout)
    buf.pos.copy_(torch.tensor([-(1 << 30), 1 << 30, 5, -1, 1 << 24], dtype=torch.int32)[:, None].expand(-1, kc))
    buf.count.copy_(torch.tensor([1 << 30, kc + 7, -5, 3, kc], dtype=torch.int32))
    buf.nv.copy_(torch.tensor([1 << 30, -9, 4000, 4001, 3999], dtype=torch.int32))
    buf.tq.copy_(torch.tensor([-1, 1 << 30, ONE, 0, 1 << 17], dtype=torch.int32))
    guard = torch.full((4096,), 7.5, device=DEV)             # (allocated after out: what lies behind it stays)
    assert _lib.load().sa_wsola_ola(_f(buf.wav), _f(buf.pos), _f(buf.count), _f(buf.tq), _f(buf.nv), _f(buf.hann),
                                    buf.B, buf.N, buf.Nout, _f(buf.out), _lib.stream()) == 0
    torch.cuda.synchronize()
    out = buf.out.cpu()
    assert not torch.isnan(out).any() and bool((guard == 7.5).all())
    assert not out[1].any() and not out[2].any()              # no valid sample; no frame
    assert torch.equal(out[3, 3 * H:], torch.zeros(buf.Nout - 3 * H))      # frames from the count on are zero
    assert float(out.abs().max()) <= float(buf.wav.abs().max()) * (1.0 + 2.0 ** -22)     # (the two weights sum to 1)


@gpu
def test_entry_points_refuse_before_any_launch():
    from speech_anonymization_amd import _lib, ops
    lib, st = _lib.load(), _lib.stream()
    E = -errno.EINVAL
    buf = Buffers(CASES["batch"])
    B, N, Nout = buf.B, buf.N, buf.Nout
    a = {"wav": buf.wav, "tq": buf.tq, "nv": buf.nv, "hann": buf.hann, "ws": buf.ws, "out": buf.out, "pos": buf.pos,
         "count": buf.count, "n_out": buf.n_out}

    def calls(B=B, N=N, Nout=Nout, **swap):
        p = {k: _f(swap.get(k, v)) for k, v in a.items()}
        return {"quant": lambda: lib.sa_wsola_quant(p["wav"], p["nv"], B, N, p["ws"], st),
                "search": lambda: lib.sa_wsola_search(p["ws"], p["tq"], p["nv"], B, N, Nout, p["pos"], p["count"],
                                                      p["n_out"], st),
                "ola": lambda: lib.sa_wsola_ola(p["wav"], p["pos"], p["count"], p["tq"], p["nv"], p["hann"], B, N, Nout,
                                                p["out"], st),
                "all": lambda: lib.sa_wsola(p["wav"], p["tq"], p["nv"], p["hann"], B, N, Nout, p["ws"], p["out"],
                                            p["pos"], p["count"], p["n_out"], st)}

    takes = {"quant": ("wav", "nv", "ws"), "search": ("ws", "tq", "nv", "pos", "count", "n_out"),
             "ola": ("wav", "pos", "count", "tq", "nv", "hann", "out"), "all": tuple(a)}
    for fn, names in takes.items():
        for name in names:
            assert calls(**{name: None})[fn]() == E, (fn, name)
        for kw in ({"B": 0}, {"B": 65536}, {"B": -1}, {"N": 0}, {"N": (1 << 24) + 1}):
            assert calls(**kw)[fn]() == E, (fn, kw)
        if fn != "quant":
            for kw in ({"Nout": 0}, {"Nout": (1 << 25) + 1}, {"Nout": -4}):
                assert calls(**kw)[fn]() == E, (fn, kw)
    for fn in ("ola", "all"):                                 # out aliasing wav, whole or in part
        assert calls(out=buf.wav)[fn]() == E
        assert calls(out=buf.wav.view(-1)[N * B - 4:])[fn]() == E
    torch.cuda.synchronize()
    assert buf.untouched()
    # the binding: shapes, dtypes, strides, before the library is asked
    q = torch.zeros(B, N, dtype=torch.int16, device=DEV)
    for call in (lambda: ops.wsola_quant(buf.wav.double(), buf.nv), lambda: ops.wsola_quant(buf.wav.t(), buf.nv),
                 lambda: ops.wsola_quant(buf.wav, buf.nv.long()), lambda: ops.wsola_quant(buf.wav, buf.nv[:3]),
                 lambda: ops.wsola_quant(buf.wav[0], buf.nv), lambda: ops.wsola_quant(buf.wav, buf.nv, buf.ws[:100]),
                 lambda: ops.wsola_search(q.int(), buf.tq, buf.nv, Nout), lambda: ops.wsola_search(q, buf.tq, buf.nv, 0),
                 lambda: ops.wsola_search(q, buf.tq.float(), buf.nv, Nout),
                 lambda: ops.wsola_search(q[:, ::2], buf.tq, buf.nv, Nout),
                 lambda: ops.wsola_ola(buf.wav, buf.pos[:, :-1].contiguous(), buf.count, buf.tq, buf.nv, Nout),
                 lambda: ops.wsola_ola(buf.wav, buf.pos, buf.count, buf.tq, buf.nv, (1 << 25) + 1),
                 lambda: ops.wsola(buf.wav, buf.tq[:2], buf.nv, Nout), lambda: ops.wsola(buf.wav.cpu(), buf.tq, buf.nv, Nout)):
        with pytest.raises(_lib.SaHipError):
            call()


# ---------------------------------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------------------------------
@gpu
def test_class_gives_the_duration_exactly_and_copies_nothing_to_the_host():
    wav, nv, _, _ = CASES["batch"]
    N = wav.shape[1]
    wd, lens = _dev(wav, torch.float32), torch.tensor([v / N for v in nv], dtype=torch.float32)     # (on the CPU)
    for tempo in (0.5, 0.8, 1.0, 1.25, 2.0):
        ts = timescale.TimeScaler(tempo)
        out, lens_out = ts(wd, lens)
        want = [R.out_len(v, R.q_of(tempo)) for v in nv]
        tq, n_out, count, jumps = (v.cpu().tolist() for v in ts.last)
        assert n_out == want and out.shape == (5, max(want)) and tq == [R.q_of(tempo)] * 5
        assert lens_out.is_cuda and lens_out.cpu().tolist() == [float(np.float32(v / max(want))) for v in want]
        ref = [R.wsola(wav[b], nv[b], R.q_of(tempo), max(want)) for b in range(5)]
        assert count == [r[3] for r in ref] and jumps == [R.jumps(r[2]) for r in ref]
        assert (out.cpu().numpy().view(np.uint32) == np.stack([r[0] for r in ref]).view(np.uint32)).all()
    ts = timescale.TimeScaler(tempo_range=(0.8, 1.25), seed=5)
    first, _ = ts(wd, lens)                                  # (warm-up: the library is loaded, the window is made)
    drawn = ts.last[0].cpu().tolist()
    torch.cuda.synchronize()
    again = timescale.TimeScaler(tempo_range=(0.8, 1.25), seed=5)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                  # a device-to-host copy raises from here on
    try:
        second, lens2 = again(wd, lens)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(_bits(first), _bits(second)) and again.last[0].cpu().tolist() == drawn
    assert len(set(drawn)) > 1 and all(52429 <= v <= 81920 for v in drawn)
    third, _ = ts(wd, lens)                                  # the second call of one object draws anew
    assert ts.calls == 2 and ts.last[0].cpu().tolist() != drawn
    dev_lens, _ = timescale.TimeScaler(0.8)(wd, lens.to(DEV))                 # lengths on the device are taken too
    assert torch.equal(_bits(dev_lens), _bits(timescale.TimeScaler(0.8)(wd, lens)[0]))


@gpu
@pytest.mark.parametrize("tempo", R.F0_TEMPOS)
def test_the_pitch_stays(tempo):
    from speech_anonymization_amd import ops
    assert DELTA["f0_bar_hz"] == pytest.approx(2.0 * (DELTA["f0_delta_hz"] + DELTA["tracker_delta_hz"]))
    wav, fundamentals = R.f0_rows()
    wd, ones = wav.to(DEV), torch.ones(wav.shape[0], device=DEV)
    out, lens_out = timescale.TimeScaler(tempo)(wd, torch.ones(wav.shape[0]))
    assert out.shape[1] == DELTA[f"tempo_{tempo:g}"]["n_out"] and bool((lens_out == 1).all())
    mean_in = ops.pitch_ratio(ops.yin_f0(wd), ones, wav.shape[1])[1].cpu()
    mean_out = ops.pitch_ratio(ops.yin_f0(out), ones, out.shape[1])[1].cpu()
    print("tempo", tempo, "mean F0 in", mean_in.tolist(), "out", mean_out.tolist(), "bar", DELTA["f0_bar_hz"])
    assert float((mean_out - mean_in).abs().max()) <= DELTA["f0_bar_hz"]
    assert float((mean_in.double() - torch.tensor(fundamentals, dtype=torch.float64)).abs().max()) <= DELTA["f0_bar_hz"]


# ---------------------------------------------------------------------------------------------------
# the command line and the recipe
# ---------------------------------------------------------------------------------------------------
@gpu
def test_anonymize_tempo_mode_with_the_f0_report(tmp_path, capsys):
    res = anon_cli.run(capsys, ["--device", DEV, "--synthetic", "4", "--out_dir", str(tmp_path), "--tempo", "0.8",
                                "--report_f0", "true"])
    assert res["tempo"] is True and res["n_iter"] is None
    assert not {"pitch_norm", "model_type", "recon_ckpt", "mcadams", "resynth", "modspec", "tempo_range", "seed"} & set(res)
    assert sorted(os.listdir(tmp_path)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    for u in res["utterances"]:
        assert {"id", "samples", "peak", "tempo", "samples_in", "frames", "jumps", "f0_mean_hz", "voiced_share"} <= set(u)
        assert u["tempo"] == 52429 / 65536 and u["samples"] == R.out_len(u["samples_in"], 52429)
        assert u["frames"] == (u["samples"] - 1) // 160 + 1 and 0 <= u["jumps"] < u["frames"] and 0 < u["peak"] < 4
        assert 60.0 < u["f0_mean_hz"] < 400.0 and u["voiced_share"] > 0.5     # measured over the samples written


@gpu
def test_anonymize_tempo_range_in_a_child_and_an_older_mode_twice(tmp_path):
    """a drawn tempo per utterance in a fresh child; and two children of a mode that was there before write the same
    bytes and print the same line, none of the new keys in it"""
    res = anon_cli.run_child(["--device", DEV, "--synthetic", "4", "--out_dir", str(tmp_path / "t"), "--tempo_min",
                              "0.8", "--tempo_max", "1.25", "--seed", "11"])
    assert res["tempo"] is True and res["tempo_range"] == [0.8, 1.25] and res["seed"] == 11
    tempos = [u["tempo"] for u in res["utterances"]]
    assert len(set(tempos)) > 1 and all(0.8 <= t <= 1.25 for t in tempos)
    lines = []
    for name in ("a", "b"):
        line = anon_cli.run_child(["--device", DEV, "--synthetic", "3", "--out_dir", str(tmp_path / name), "--mcadams",
                                   "0.8"])
        assert line["mcadams"] is True and not {"tempo", "tempo_range"} & set(line)
        assert not {"tempo", "samples_in", "frames", "jumps"} & set(line["utterances"][0])
        lines.append(dict(line, out_dir=None))
    assert lines[0] == lines[1]
    for fn in sorted(os.listdir(tmp_path / "a")):
        with open(tmp_path / "a" / fn, "rb") as fa, open(tmp_path / "b" / fn, "rb") as fb:
            assert fa.read() == fb.read(), fn


@gpu
def test_recipe_trains_one_epoch(tmp_path):
    """a fresh child process, under a time limit; no error bar: one epoch on 16 synthetic utterances"""
    out = tmp_path / "tempo_recipe"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gender_classifier_train_tempo.py"),
                        os.path.join(ROOT, "speechbrain_configs", "gender_classifier_tempo.yaml"), "--device", DEV,
                        "--output_folder", str(out), "--synthetic", "16", "--number_of_epochs", "1",
                        "--tempo_min", "0.8", "--tempo_max", "1.25"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["tempo_mode"] is True and summary["tempo_range"] == [0.8, 1.25] and summary["seed"] == 1
    assert np.isfinite(summary["test_loss"]) and 0.0 <= summary["test_error"] <= 1.0
