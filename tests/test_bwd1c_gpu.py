"""ops.bwd1C (sa_bwd1C: the backward of the 32 -> 1 layer in one launch) against the two launches it
replaces, ops.conv1toC with the [InstanceNorm -> swish] backward epilogue and ops.wgrad1C with the
prologue: the data gradient, the statistics slabs and the summed weight gradient, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
# shorter than a tile; a partial statistics tile and a partial MFMA tile; a chunk boundary inside an
# utterance with a ragged tail; exact multiples
LENGTHS = [100, 512 * 2 + 37, 2048 + 256 + 5, 4096]


def _inputs(Ln, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda:0")
    u = torch.randn(B, Ln, generator=g).to(dev)
    v = torch.randn(B, Ln, 32, generator=g).to(dev, dtype)
    w = (torch.randn(1, 32, 15, generator=g) * 0.2).to(dev)
    s1 = (0.5 + torch.rand(B, 32, generator=g)).to(dev)
    t1 = (0.3 * torch.randn(B, 32, generator=g)).to(dev)
    mean = (0.1 * torch.randn(B, 32, generator=g)).to(dev)
    rstd = (0.5 + torch.rand(B, 32, generator=g)).to(dev)
    return u, v, w, s1, t1, mean, rstd


def _two_launches(u, v, w, s1, t1, mean, rstd, flip):
    from speech_anonymization_amd import ops
    g, st = ops.conv1toC(u, w, None, v.dtype, flip=flip, want_stats=True,
                         ep=dict(x=v, s1=s1, t1=t1, mean=mean, rstd=rstd))
    dw = ops.wgrad1C(u, v, torch.empty_like(w), flip=flip, s1=s1, t1=t1, swish=True, chunk=2048)
    return g, st, dw


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Ln", LENGTHS)
def test_bwd1c_equals_dgrad_plus_wgrad(Ln, dtype):
    from speech_anonymization_amd import ops
    args = _inputs(Ln, dtype, seed=Ln)
    g0, st0, dw0 = _two_launches(*args, flip=True)
    u, v, w, s1, t1, mean, rstd = args
    g1, st1, dw1 = ops.bwd1C(u, v, w, torch.empty_like(w), s1, t1, mean, rstd, flip=True, chunk=2048)
    torch.cuda.synchronize()
    assert g1.dtype == g0.dtype and g1.shape == g0.shape and st1.shape == st0.shape
    assert torch.equal(g1, g0)
    assert torch.equal(st1, st0)
    assert torch.equal(dw1, dw0)
    assert float(g0.float().abs().max()) > 0 and float(dw0.abs().max()) > 0


def test_bwd1c_unflipped_taps():
    """flip=False is accepted with the prologue (same comparison); accumulate adds to the destination"""
    from speech_anonymization_amd import ops
    args = _inputs(2048 + 256 + 5, torch.float32, seed=7)
    g0, st0, dw0 = _two_launches(*args, flip=False)
    u, v, w, s1, t1, mean, rstd = args
    base = torch.full_like(w, 0.25)
    g1, st1, dw1 = ops.bwd1C(u, v, w, base.clone(), s1, t1, mean, rstd, flip=False, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(g1, g0) and torch.equal(st1, st0)
    assert torch.equal(dw1, base + dw0)


def test_bwd1c_refuses_a_missing_prologue_and_a_split_statistics_tile():
    """no prologue (flip=False or True): the entry point has nothing to share between the two results and
    returns -EINVAL, as it does for a chunk that would split a 512-position statistics tile"""
    from speech_anonymization_amd import _lib as L, ops
    u, v, w, s1, t1, mean, rstd = _inputs(100, torch.float32, seed=1)
    lib = L.load()
    g, st, slabs = torch.empty_like(v), torch.empty(B, 1, 32, 2, device=v.device), torch.empty(B, 480, device=v.device)

    def call(chunk, flip, s1_, t1_, mean_, rstd_):
        return lib.sa_bwd1C(L.F32, L.ptr(u), L.ptr(v), L.ptr(w), L.ptr(g), L.ptr(st), L.ptr(slabs), B, 100, chunk,
                            flip, L.ptr(s1_), L.ptr(t1_), L.ptr(mean_), L.ptr(rstd_), L.stream())

    assert call(2048, 0, None, None, None, None) == -22
    assert call(2048, 1, None, None, mean, rstd) == -22
    assert call(2048, 1, s1, t1, None, None) == -22
    assert call(256, 1, s1, t1, mean, rstd) == -22
    assert call(2048, 1, s1, t1, mean, rstd) == 0
    with pytest.raises(L.SaHipError):
        ops.bwd1C(u, v, w, torch.empty_like(w), None, None, None, None, flip=False)
    torch.cuda.synchronize()
