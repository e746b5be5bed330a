"""CPU: tests/ref64.py (the fp64 arbiter of tests/test_losses_gpu.py) against torch autograd in
fp64, the reference's own outputs under tests/golden/ and hand values; and where the oracle's
cosine (the installed torch's) and the reference's pinned torch 1.10 part ways."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as OL
from tests import ref64

U = 2.0 ** -24            # unit roundoff of fp32


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _close(a, b, tol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- recon / classifier losses / log-softmax / pooling against autograd, fp64, 1e-12 ----------
@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_recon_equals_autograd(kind):
    a, b = _rand(7, 33, seed=1).requires_grad_(True), _rand(7, 33, seed=2)
    with torch.no_grad():
        b[2] = a[2]                                   # exact zeros of a - b
    ref = F.l1_loss(a, b) if kind == "l1" else F.mse_loss(a, b)
    (g,) = torch.autograd.grad(ref, a)
    loss, grad = ref64.recon(a, b, kind)
    assert _close(loss, ref.detach(), 1e-12) and _close(grad, g, 1e-12)
    if kind == "l1":
        assert float(grad[2].abs().max()) == 0.0      # sign(0) = 0


@pytest.mark.parametrize("NC", [2, 3])
def test_log_softmax_and_cls_losses_equal_autograd(NC):
    x = _rand(11, NC, seed=3, scale=5.0).requires_grad_(True)
    lp = F.log_softmax(x, dim=1)
    assert _close(ref64.log_softmax(x), lp.detach(), 1e-12)
    dy = _rand(11, NC, seed=4)
    (gx,) = torch.autograd.grad(lp, x, dy)
    assert _close(ref64.log_softmax_bwd(dy, lp), gx, 1e-12)
    # saturated rows stay finite
    sat = ref64.log_softmax(torch.tensor([[80.0, -80.0], [-80.0, 80.0], [5.0, 5.0]]))
    assert torch.isfinite(sat).all() and abs(float(sat[2, 0]) + math.log(2.0)) < 1e-15
    assert float(sat[0, 0]) == 0.0 and float(sat[0, 1]) == -160.0
    lpl = lp.detach().clone().requires_grad_(True)
    label = torch.arange(11) % NC
    nll = F.nll_loss(lpl, label)
    conf = F.mse_loss(lpl, torch.full_like(lpl, ref64.LOG_HALF_F32))
    (gn,) = torch.autograd.grad(nll, lpl)
    (gc,) = torch.autograd.grad(conf, lpl)
    rn, rc, dn, dc = ref64.cls_losses(lpl, label)
    assert _close(rn, nll.detach(), 1e-12) and _close(rc, conf.detach(), 1e-12)
    assert _close(dn, gn, 1e-12) and _close(dc, gc, 1e-12)
    # the target is the fp32 literal, not the double one
    assert ref64.LOG_HALF_F32 != -0.6931 and abs(ref64.LOG_HALF_F32 + 0.6931) < 0.6931 * U


@pytest.mark.parametrize("L", [2, 5, 129])
def test_stat_pool_equals_autograd(L):
    from oracle.convae import StatisticsPooling
    B, C = 2, 128
    x = _rand(B, C, L, seed=5).requires_grad_(True)
    noise = torch.rand(B, C, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    pooled = StatisticsPooling()(x.reshape(B, L, C)).squeeze(1)
    dp = _rand(B, 2 * C, seed=7)
    (gx,) = torch.autograd.grad(pooled, x, dp)
    got, _, _ = ref64.stat_pool(x)
    assert _close(got, pooled.detach(), 1e-12)
    assert _close(ref64.stat_pool_bwd(x, dp), gx, 1e-12)
    pn = StatisticsPooling(noise=noise)(x.detach().reshape(B, L, C)).squeeze(1)
    assert _close(ref64.stat_pool(x, noise=noise)[0], pn, 1e-12)
    # the quirk: pooled column j collects the flat elements f = c*L + l with f % 128 == j
    flat = x.detach().reshape(B, C * L)
    assert _close(got[:, :C], torch.stack([flat[:, j::C].mean(1) for j in range(C)], 1), 1e-12)


# ---- cosine -----------------------------------------------------------------------------------
def _generic_rows(B, S, D, seed):
    """rows with norms >= 1e-3 (here: 0.05 .. 50)"""
    x1, x2 = _rand(B, S, D, seed=seed), _rand(B, S, D, seed=seed + 1)
    s = 10.0 ** (torch.rand(B, S, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 2)) * 2 - 1)
    x1 = x1 / x1.norm(dim=2, keepdim=True) * s * 0.5
    x2 = x2 / x2.norm(dim=2, keepdim=True) * s.flip(0) * 5.0
    return x1, x2


def test_cosine_golden_and_installed_torch_on_generic_rows(golden_dir):
    z = np.load(os.path.join(golden_dir, "losses.npz"))
    loss, _, _ = ref64.cosine_loss(z["x1"], z["x2"])
    stored = float(z["cos_loss"])                       # an fp32 value
    # fp32 rounding of the stored value (1 ulp <= 2 U |v|) + the reference's own fp32 evaluation:
    # B*S rows, each 1 - cos good to ~ (D + 4) U, summed and divided by S
    B, S, D = z["x1"].shape
    assert abs(float(loss) - stored) <= 2 * U * abs(stored) + B * (D + 4) * U
    x1, x2 = _generic_rows(3, 7, 65, seed=10)
    assert float(torch.minimum(x1.norm(dim=2), x2.norm(dim=2)).min()) >= 1e-3
    x1r = x1.clone().requires_grad_(True)
    sim = F.cosine_similarity(x1r, x2, dim=2, eps=1e-6)
    ref = (1 - sim).sum() / sim.shape[1]
    (g,) = torch.autograd.grad(ref, x1r)
    loss, row, dx1 = ref64.cosine_loss(x1, x2)
    assert _close(loss, ref.detach(), 1e-12) and _close(row, (1 - sim).detach(), 1e-12)
    assert _close(dx1, g, 1e-12)


def test_cosine_degenerate_rows_follow_torch_1_10():
    """Hand values of the product clamp.  What the installed torch returns on these rows is
    deliberately not asserted: since 1.12 it clamps each norm and gives 0.0707 / x2/(eps |x2|)."""
    eps = ref64.f32_eps(1e-6)
    x1 = torch.tensor([[[1e-7, 0, 0, 0]], [[0.0, 0, 0, 0]], [[1e-4, 0, 0, 0]], [[0.0, 0, 0, 0]], [[3.0, 4, 0, 0]]],
                      dtype=torch.float64)
    x2 = torch.tensor([[[100.0, 100, 0, 0]], [[100.0, 100, 0, 0]], [[6e-5, 8e-5, 0, 0]], [[0.0, 0, 0, 0]], [[0.0, 0, 0, 0]]],
                      dtype=torch.float64)
    loss, row, dx1 = ref64.cosine_loss(x1, x2)
    cos = 1 - row[:, 0]
    # |x1| |x2| = 1e-7 * 141.4 = 1.4e-5 > eps: not clamped, the plain cosine 1/sqrt(2)
    assert abs(float(cos[0]) - math.sqrt(0.5)) < 1e-12
    # x2/(|x1||x2|) - cos x1/|x1|^2: the component along x1 cancels (1/(1e-7 sqrt 2) both times)
    g0 = torch.tensor([0.0, 100.0 / (1e-7 * math.sqrt(2e4)), 0.0, 0.0], dtype=torch.float64)
    assert _close(dx1[0, 0], -g0, 1e-9)
    # zero x1 row: cos 0, gradient x2 / eps (S = 1)
    assert float(cos[1]) == 0.0 and _close(dx1[1, 0], -x2[1, 0] / eps, 1e-14)
    # |x1| = |x2| = 1e-4: product 1e-8 < eps, clamped: cos = x1.x2 / eps, gradient x2 / eps
    assert abs(float(cos[2]) - 6e-9 / eps) < 1e-15 and _close(dx1[2, 0], -x2[2, 0] / eps, 1e-14)
    # both zero, and x2 zero: cos 0, gradient 0
    assert float(cos[3]) == 0.0 and float(dx1[3].abs().max()) == 0.0
    assert float(cos[4]) == 0.0 and float(dx1[4].abs().max()) == 0.0
    assert abs(float(loss) - float(row.sum())) < 1e-15        # S = 1


def test_oracle_cosine_agrees_with_ref64_on_generic_rows():
    """oracle.losses.cosine_similarity_loss (fp32, the installed torch's per-norm clamp) against
    the fp64 1.10 formula where the two clamps cannot differ: every row norm >= 1e-3."""
    B, S, D = 3, 7, 65
    x1, x2 = _generic_rows(B, S, D, seed=20)
    x1, x2 = x1.float(), x2.float()
    got = float(OL.cosine_similarity_loss(x1, x2))
    ref, _, _ = ref64.cosine_loss(x1, x2)
    # fp32 oracle: dot and both squared norms are D-term sums (<= D U relative to |x1||x2| each in
    # the worst summation order), a few roundings for sqrt / divide / 1 - cos: (2 D + 4) U per row,
    # B*S rows summed (each rounding <= U * partial sum <= 2 B S U) and divided by S
    bound = B * (2 * D + 4) * U + 2 * B * S * U * 2 * B
    assert abs(got - float(ref)) <= bound


# ---- cluster MI -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["losses.npz", "losses_n32.npz"])
def test_cluster_mi_reproduces_reference_vectors(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    mi, lo, hi = ref64.cluster_mi(z["X"], z["y"])
    assert abs(mi[0] - float(z["mi"])) < 1e-5 and lo[0] == mi[0] == hi[0]
    mis, _, _ = ref64.cluster_mi(z["X"], z["y"], z["idx_sets"])
    assert np.abs(mis - z["mi_list"]).max() < 1e-5


def test_cluster_mi_equals_oracle_on_fresh_case():
    g = torch.Generator().manual_seed(31)
    y = torch.arange(14) % 3
    X = torch.randn(14, 6, generator=g) + 0.5 * y[:, None].float()
    want = float(OL.cluster_mi(X, y, n_classes=3, k=2))
    mi, _, _ = ref64.cluster_mi(X, y, ncls=3, k=2)
    assert abs(mi[0] - want) < 1e-5
    # a class with fewer than k + 1 members: its anchors are 10e6, m = n - 1
    y2 = torch.tensor([0] * 2 + [1] * 12)
    want = float(OL.cluster_mi(X, y2, n_classes=2, k=3))
    mi, _, _ = ref64.cluster_mi(X, y2, ncls=2, k=3)
    assert abs(mi[0] - want) < 1e-5


def test_cluster_mi_interval_brackets_and_detects_miscounts():
    g = torch.Generator().manual_seed(32)
    y = torch.arange(64) % 2
    X = torch.randn(64, 128, generator=g) + 0.3 * y[:, None].float()
    idx = np.stack([np.random.RandomState(s).permutation(64)[:32] for s in range(20)])
    tau = ref64.distance_tau(X)
    assert 0.0 < tau < 1e-5
    mi, lo, hi = ref64.cluster_mi(X, y, idx, tau=tau)
    assert (lo <= mi).all() and (mi <= hi).all()
    mi0, lo0, hi0 = ref64.cluster_mi(X, y, idx)
    assert (lo0 == mi0).all() and (hi0 == mi0).all() and (mi0 == mi).all()
    # a huge tau makes everything undecided: the interval is then wide, never inverted
    _, lo1, hi1 = ref64.cluster_mi(X, y, idx, tau=1.0)
    assert (hi1 - lo1 > 0.5).all()
