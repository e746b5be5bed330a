"""fp64 restatements of the loss and pooling operations, written out as formulas.

The arbiter for tests/test_losses_gpu.py: every kernel of csrc/sa_head.hip / csrc/sa_mi.hip that
ends a forward pass or starts a backward pass is compared with these functions on the same fp32
inputs.  Nothing here calls the package under test or torch.nn.functional: where the installed
torch departs from the reference's pinned torch 1.10 (cosine_similarity clamps each norm
separately since 1.12; 1.10 clamps the PRODUCT of the squared norms) the 1.10 formula is written
out, because that is what the kernels implement.  tests/test_ref64_cpu.py checks this module
against torch autograd in fp64, the golden fixtures and hand values.

Inputs may be torch tensors or numpy arrays of any float type; everything is widened to fp64
first, so "the same fp32 inputs" are seen exactly.
"""
import math

import numpy as np
import torch

# The confusion target as the kernel (and torch's fp32 MSELoss) sees it: the reference's literal
# -0.6931 rounded to fp32, widened -- not the double -0.6931 (they differ by 1.3e-8).
LOG_HALF_F32 = float(np.float32(-0.6931))


def _t(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.detach().cpu().double()


def f32_eps(eps):
    """a python-float eps as an fp32 kernel receives it (ATen casts the double argument to the
    tensor's scalar type; the HIP kernels hold 1e-6f / 1e-16f literals)"""
    return float(np.float32(eps))


# ---------------------------------------------------------------------------------------------
def recon(a, b, kind):
    """mean |a-b| ("l1") or mean (a-b)^2 ("mse") over every element -> (loss, d loss / d a).
    L1: sign(0) = 0 (what torch's l1_loss backward does and what zero-padded frames need)."""
    a, b = _t(a), _t(b)
    d, n = a - b, a.numel()
    if kind == "l1":
        return d.abs().sum() / n, torch.sign(d) / n
    assert kind == "mse"
    return (d * d).sum() / n, 2.0 * d / n


def log_softmax(x):
    """over the last dimension of [M, N]"""
    x = _t(x)
    mx = x.max(dim=1, keepdim=True)[0]
    return x - (mx + torch.log(torch.exp(x - mx).sum(dim=1, keepdim=True)))


def log_softmax_bwd(dy, y):
    """dx = dy - exp(y) * sum_n dy   (y = log_softmax(x))"""
    dy, y = _t(dy), _t(y)
    return dy - torch.exp(y) * dy.sum(dim=1, keepdim=True)


def cls_losses(logp, label):
    """NLLLoss(mean) and MSELoss(logp, float32(-0.6931)) on logp [B, NC]
    -> (nll, conf, d nll / d logp, d conf / d logp)."""
    logp = _t(logp)
    label = torch.as_tensor(label).cpu().long()
    B, NC = logp.shape
    hit = torch.zeros(B, NC, dtype=torch.float64)
    hit[torch.arange(B), label] = 1.0
    nll = -(logp * hit).sum() / B
    d = logp - LOG_HALF_F32
    return nll, (d * d).sum() / (B * NC), -hit / B, 2.0 * d / (B * NC)


# ---------------------------------------------------------------------------------------------
def cosine_rows(x1, x2, eps=1e-6):
    """torch 1.10's cosine_similarity over the last dimension:
         cos = x1.x2 / sqrt(max(|x1|^2 |x2|^2, eps^2))          (the product is clamped)
    -> (cos, na = |x1|^2, nb = |x2|^2, clamped mask)."""
    x1, x2 = _t(x1), _t(x2)
    e2 = f32_eps(eps) ** 2
    dot, na, nb = (x1 * x2).sum(-1), (x1 * x1).sum(-1), (x2 * x2).sum(-1)
    clamped = na * nb < e2
    return dot / torch.sqrt(torch.clamp_min(na * nb, e2)), na, nb, clamped


def cosine_loss(x1, x2, eps=1e-6):
    """CosineSimilarityLoss on [B, S, D]: sum_{b,s}(1 - cos) / S  (divides by S, not B*S)
    -> (loss, per-row loss [B, S], d loss / d x1).
    Gradient = autograd of the 1.10 formula: clamp_min passes no gradient below the bound, so
      not clamped: dx1 = -(1/S) (x2 / (|x1||x2|) - cos x1 / |x1|^2)
      clamped    : dx1 = -(1/S) x2 / eps."""
    x1, x2 = _t(x1), _t(x2)
    S = x1.shape[1]
    cos, na, nb, clamped = cosine_rows(x1, x2, eps)
    den = torch.sqrt(torch.clamp_min(na * nb, f32_eps(eps) ** 2)).unsqueeze(-1)
    g = x2 / den
    corr = cos.unsqueeze(-1) * x1 / torch.where(clamped, torch.ones_like(na), na).unsqueeze(-1)
    g = torch.where(clamped.unsqueeze(-1), g, g - corr)
    row = 1.0 - cos
    return row.sum() / S, row, -g / S


# ---------------------------------------------------------------------------------------------
def pairwise_cosine_dists(X, eps=1e-8, dtype=torch.float64):
    """d[i, j] = 1 - x_i.x_j / sqrt(max(|x_i|^2 |x_j|^2, eps^2)), diagonal 0.
    fp64: every dot product is an elementwise product summed along the last axis, so the value
    depends on the pair's data only -- duplicated rows give bit-identical distances and the matrix
    is exactly symmetric (a BLAS matmul guarantees neither).  dtype=float32 is the plain fp32
    evaluation (matmul) used to MEASURE the fp32 error of a pool."""
    if dtype == torch.float32:
        X = (torch.from_numpy(X) if isinstance(X, np.ndarray) else X).detach().cpu().float()
        G = X @ X.t()
        nrm = (X * X).sum(1)
        e2 = torch.tensor(np.float32(eps) * np.float32(eps))
    else:
        X = _t(X)
        G = torch.stack([(X[i:i + 1] * X).sum(1) for i in range(X.shape[0])])
        nrm = torch.diagonal(G).clone()
        e2 = torch.tensor(f32_eps(eps) ** 2, dtype=torch.float64)
    d = 1.0 - G / torch.sqrt(torch.maximum(nrm[:, None] * nrm[None, :], e2))
    d.fill_diagonal_(0.0)
    return d


def cluster_mi(X, y, idx=None, ncls=2, k=3, tau=0.0):
    """Ross (2014) k-NN mutual information between the rows of X [N, D] and labels y [N], in
    bits, for every index set of idx [iters, n] (None: one set, rows 0..N-1):
      anchor_i = (k+1)-th smallest same-class distance (self included; other classes count 10e6)
      m_i      = #{j : d_ij <= anchor_i} - 1
      MI       = (psi(n) - sum_c n_c/n psi(n_c) + psi(k) - mean_i psi(m_i)) / ln 2
    -> (mi [iters], mi_lo [iters], mi_hi [iters]).
    [mi_lo, mi_hi] is the admissible interval of an evaluation whose distances err by at most tau:
    both d_ij and the anchor (an order statistic: 1-Lipschitz in the sup norm) move by <= tau, so
    every j with 0 < |d_ij - anchor_i| <= 2 tau is undecided.  mi_hi counts all undecided ones
    out (smallest m), mi_lo all of them in (largest m).  tau = 0: mi_lo == mi == mi_hi."""
    y = torch.as_tensor(y).cpu().long()
    dpool = pairwise_cosine_dists(X)
    N = dpool.shape[0]
    idx = torch.arange(N)[None] if idx is None else torch.as_tensor(idx).cpu().long()
    big = torch.tensor(10e6, dtype=torch.float64)
    out = []
    for s in idx:
        n = s.numel()
        d, lab = dpool[s][:, s], y[s]
        same = lab[:, None] == lab[None, :]
        anchor = torch.sort(torch.where(same, d, big), dim=1)[0][:, k:k + 1]
        diff = d - anchor
        m = (diff <= 0).sum(1) - 1
        m_min = ((diff == 0) | (diff < -2.0 * tau)).sum(1) - 1
        m_max = (diff <= 2.0 * tau).sum(1) - 1
        cnt = torch.tensor([float((lab == c).sum()) for c in range(ncls)], dtype=torch.float64)
        const = (torch.digamma(torch.tensor(float(n), dtype=torch.float64))
                 - (cnt / n * torch.digamma(cnt)).sum()
                 + torch.digamma(torch.tensor(float(k), dtype=torch.float64)))
        out.append([float((const - torch.digamma(v.double()).mean()) / math.log(2.0))
                    for v in (m, m_max, m_min)])
    out = np.asarray(out, dtype=np.float64)
    return out[:, 0], out[:, 1], out[:, 2]


def distance_tau(X, eps=1e-8, margin=8.0):
    """margin x the largest |d_fp32 - d_fp64| over the pool, d_fp32 being the plain fp32 CPU
    evaluation of the same formula.  Measured from the reference side only."""
    d64 = pairwise_cosine_dists(X, eps)
    d32 = pairwise_cosine_dists(X, eps, dtype=torch.float32).double()
    return margin * float((d32 - d64).abs().max())


# ---------------------------------------------------------------------------------------------
def stat_pool(xbn, noise=None, eps=1e-5):
    """The classifier's statistics pooling with the reference's reshape quirk: xbn [B, C, L]
    (channel-major memory) is REINTERPRETED as [B, L, C], then mean / unbiased std over dim 1:
      pooled [B, 2C] = (mean (+ eps ((1-9) noise + 9)), std + eps)
    -> (pooled, mean [B, C], std [B, C])."""
    x = _t(xbn)
    B, C, L = x.shape
    v = x.reshape(B, L, C)
    mean = v.sum(1) / L
    std = torch.sqrt(((v - mean[:, None, :]) ** 2).sum(1) / (L - 1))
    m = mean if noise is None else mean + eps * ((1 - 9) * _t(noise) + 9)
    return torch.cat([m, std + eps], dim=1), mean, std


def stat_pool_bwd(xbn, dpooled):
    """d xbn [B, C, L] for upstream dpooled [B, 2C]:
      g = dmean / L + dstd (x - mean) / ((L-1) std)   in the reinterpreted [B, L, C] view.
    Needs std > 0 in every pooled column (at zero variance torch's sqrt backward is non-finite)."""
    x, dp = _t(xbn), _t(dpooled)
    B, C, L = x.shape
    _, mean, std = stat_pool(x)
    v = x.reshape(B, L, C)
    g = dp[:, None, :C] / L + dp[:, None, C:] * (v - mean[:, None, :]) / ((L - 1) * std[:, None, :])
    return g.reshape(B, C, L)
