"""The kernels every training test ends in -- sa_recon_loss, sa_log_softmax(_bwd), sa_cls_losses,
sa_cosine_loss, sa_cluster_mi, sa_pool_fwd / _gather / _fin / _bwd -- and the loss modules on top,
against tests/ref64.py (fp64 formulas) on the same fp32 inputs, at the training shapes and at the
edges of their loops.  Every tolerance states the roundings it counts; none is taken from what a
kernel returned.  U = 2^-24 is the unit roundoff of fp32 (one rounding errs by <= U relative)."""
import math

import numpy as np
import pytest
import torch

from tests import ref64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def dev():
    return torch.device("cuda:0")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ulp32(ref):
    """spacing of fp32 at |ref| (fp64 array in, fp64 array out)"""
    return np.spacing(np.abs(np.asarray(ref, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def rel_mse(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-30))


def offset_view(t):
    """the same values as a contiguous device view whose pointer is 4 bytes past a 16-byte boundary"""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev())
    base[1:] = t.reshape(-1).to(dev())
    v = base[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ================================================================================================
# sa_recon_loss
# ================================================================================================
# n4 = 0 (1, 2, 3), tail of 1 (5), 3 (1023, 5 160 963), exactly one pass of 512 x 256 float4
# (524 288), one float4 into the second pass (524 292), the benchmark step 32 x 1008 x 80, ten passes
RECON_N = [1, 2, 3, 5, 1023, 524288, 524292, 2580480, 5160963]


def recon_inputs(kind, n):
    g = gen(1000 + n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if kind == "mse":                                   # magnitudes up to 1e4
        a = a * 10.0 ** (4.0 * torch.rand(n, generator=g))
    if n >= 5:                                          # zero-padded frames: a == b exactly
        lo = n // 3
        b[lo:lo + max(1, n // 5)] = a[lo:lo + max(1, n // 5)]
    return a, b


@pytest.mark.parametrize("n", RECON_N)
@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_recon_loss_sizes(kind, n):
    from speech_anonymization_amd import ops
    a, b = recon_inputs(kind, n)
    want, gref = ref64.recon(a, b, kind)
    want, gref = float(want), gref.numpy()
    ad, bd = a.to(dev()), b.to(dev())
    loss, grad = ops.recon_loss(ad, bd, kind)
    loss2, grad2 = ops.recon_loss(ad, bd, kind)
    loss3, none = ops.recon_loss(ad, bd, kind, want_grad=False)
    torch.cuda.synchronize()
    got, g = float(loss), grad.cpu().numpy().astype(np.float64)
    err = abs(got - want) / max(abs(want), 1e-300)
    print(f"recon {kind} n={n}: loss {got:.9g} ref {want:.9g} rel err {err / U:.3f} U")
    # loss: d = fl(a - b) [1 rounding, U relative], squared for MSE [the error doubles: 2 U], summed
    # in fp64 [n * 2^-53 <= 6e-10 at n = 5.2e6: nothing], one final rounding to fp32 [U]: <= 3 U
    assert err <= 3 * U
    if kind == "l1":
        # +-(1.0f / float(n)) or 0, nothing else: bit-equal
        inv = np.float32(1.0) / np.float32(n)
        exp = np.sign(gref).astype(np.float32) * inv
        assert np.array_equal(grad.cpu().numpy(), exp)
        if n >= 5:
            assert (exp == 0).sum() >= max(1, n // 5)   # the a == b block is in the data
    else:
        # 2*fl(a-b)*fl(1/n) rounded: three roundings (a-b, 1/n, the product; 2*d is exact), each at
        # most one ulp of the result: 4 ulp leaves one of margin
        e = np.abs(g - gref) / ulp32(gref)
        print(f"  grad: max {e.max():.3f} ulp")
        assert e.max() <= 4.0
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert none is None and torch.equal(loss, loss3)


@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_recon_modules(kind):
    """ReconLoss / L1Loss / MSELoss: upstream factor, non-contiguous, bf16, no-grad path and a
    contiguous view at a misaligned storage offset (which the kernel itself refuses)."""
    from speech_anonymization_amd import losses, ops
    from speech_anonymization_amd._lib import SaHipError
    mod = losses.L1Loss() if kind == "l1" else losses.MSELoss()
    assert isinstance(mod, losses.ReconLoss) and mod.kind == kind
    B, T, Fd = 3, 37, 80
    a, b = torch.randn(B, T * Fd, generator=gen(61)), torch.randn(B, T * Fd, generator=gen(62))
    b[1, 100:900] = a[1, 100:900]
    want, gref = ref64.recon(a, b, kind)
    # gradient * 0.1: the kernel's own roundings (l1: 1/n = 1; mse: 3), float32(0.1) and the product
    gtol = (3 if kind == "l1" else 5) * U + U

    def check(pred, target, want, gref, tol_loss=3 * U, tol_g=gtol):
        loss = mod(pred, target)
        assert loss.shape == () and loss.dtype == torch.float32
        assert abs(float(loss.detach()) - float(want)) <= tol_loss * abs(float(want))
        (0.1 * loss).backward()
        assert pred.grad.shape == pred.shape and pred.grad.dtype == pred.dtype
        e = (pred.grad.double().cpu() - 0.1 * gref).abs().max() / (0.1 * gref).abs().max()
        assert float(e) <= tol_g
        return loss

    p = a.to(dev()).requires_grad_(True)
    l1 = check(p, b.to(dev()), want, gref)
    # no-grad path: the same loss bits, no graph
    l2 = mod(a.to(dev()), b.to(dev()))
    assert torch.equal(l1.detach(), l2) and not l2.requires_grad
    # transposed (non-contiguous) prediction and target
    pt = a.t().contiguous().to(dev()).t().requires_grad_(True)
    assert not pt.is_contiguous()
    check(pt, b.t().contiguous().to(dev()).t(), want, gref)
    # bf16 prediction: the loss of the widened values; the gradient comes back in bf16 (2^-9 relative)
    ab = a.to(torch.bfloat16)
    wb, gb = ref64.recon(ab.float(), b, kind)
    pb = ab.to(dev()).requires_grad_(True)
    check(pb, b.to(dev()), wb, gb, tol_g=2.0 ** -8)
    # misaligned contiguous views: the C entry point refuses them (-22), the wrapper copies
    pm, tm = offset_view(a).detach().requires_grad_(True), offset_view(b)
    assert pm.data_ptr() % 16 == 4
    check(pm, tm, want, gref)
    fa = offset_view(a.reshape(-1))
    lo, go = ops.recon_loss(fa, b.reshape(-1).to(dev()), kind)
    lr, gr = ops.recon_loss(a.reshape(-1).to(dev()), offset_view(b.reshape(-1)), kind)
    torch.cuda.synchronize()
    assert torch.equal(lo, l1.detach().reshape(1)) and torch.equal(lr, lo) and torch.equal(go, gr)
    import ctypes as C
    from speech_anonymization_amd import _lib as L
    lib = L.load()
    ws = torch.empty(lib.sa_loss_workspace_bytes() // 8, dtype=torch.float64, device=dev())
    out = torch.empty(1, device=dev())
    rc = lib.sa_recon_loss(C.c_void_p(fa.data_ptr()), L.ptr(tm), C.c_longlong(fa.numel()), 0, None,
                           L.ptr(out), L.ptr(ws), L.stream())
    assert rc == -22
    with pytest.raises(SaHipError):
        L.check(rc, "sa_recon_loss")


# ================================================================================================
# sa_log_softmax, sa_log_softmax_bwd, sa_cls_losses
# ================================================================================================
def cls_logits(B, NC, scale):
    x = torch.randn(B, NC, generator=gen(200 + B)) * scale
    special = [[80.0, -80.0], [-80.0, 80.0], [5.0, 5.0]]
    for i, row in enumerate(special[:B]):               # saturated both ways, and an exact tie
        x[B - 1 - i, :2] = torch.tensor(row)
    return x


def check_cls(B, NC, scale):
    from speech_anonymization_amd import ops
    x = cls_logits(B, NC, scale)
    Lmax = x.double().abs().max(1, keepdim=True)[0]      # per row: a saturated row must not widen the others' bound
    LP = ops.log_softmax(x.to(dev()))
    torch.cuda.synchronize()
    lp_ref = ref64.log_softmax(x)
    # logp = x - (mx + logf(sum expf(x - mx))), expf / logf good to 2 ulp = 4 U relative:
    #   t = x - mx          1 rounding: U |t|, which expf turns into U |t| e^t <= U / e relative
    #   s = sum expf(t)     4 U + U/e + (NC-1) U relative   (s in [1, NC])
    #   l = logf(s)         4 U ln NC + the relative error of s
    #   lse = mx + l        1 rounding: U (Lmax + ln NC)
    #   logp = x - lse      1 rounding: U (2 Lmax + ln NC)
    # NC <= 3: U (4 + 0.37 + 2 + 4.4 + 2.2 + 3 Lmax) <= U (14 + 3 Lmax), Lmax = the row's largest |logit|
    tol_row = U * (14.0 + 3.0 * Lmax)
    e_lp = (LP.double().cpu() - lp_ref).abs()
    worst = int((e_lp / tol_row).max(1)[0].argmax())
    print(f"cls B={B} NC={NC} scale={scale}: worst row {worst}: logp err {float(e_lp[worst].max()) / U:.2f} U "
          f"(bound {float(tol_row[worst]) / U:.0f} U)")
    assert torch.isfinite(LP).all() and bool((e_lp <= tol_row).all())
    tol_lp = float(tol_row.max())
    lpc = LP.cpu()
    labels = [torch.randint(0, NC, (B,), generator=gen(300 + B)), torch.zeros(B, dtype=torch.long),
              torch.ones(B, dtype=torch.long)]
    for lab in labels:
        out, dn, dc = ops.cls_losses(LP, lab.to(dev()))
        out2, n1, n2 = ops.cls_losses(LP, lab.to(dev()), want_grad=False)
        torch.cuda.synchronize()
        assert n1 is None and n2 is None and torch.equal(out, out2)
        # against ref64 on the kernel's own fp32 logp: the loss kernel alone
        nll, conf, dnr, dcr = ref64.cls_losses(lpc, lab)
        # dnll: -1.0f / float(B) at the label, 0 elsewhere: bit-equal
        exp = (dnr.numpy() != 0).astype(np.float32) * (np.float32(-1.0) / np.float32(B))
        assert np.array_equal(dn.cpu().numpy(), exp)
        # dconf = 2 fl(logp + 0.6931f) / float(B NC): two roundings (2*d is exact) = 2 U, margin 1
        e = (dc.double().cpu() - dcr).abs() / dcr.abs().clamp_min(1e-300)
        assert float(e.max()) <= 3 * U
        # nll: fp32 values summed in fp64 (exact to 2^-53 each), /B, one rounding: U; margin 1
        assert abs(float(out[0]) - float(nll)) <= 2 * U * abs(float(nll))
        # conf: d has one rounding (U), squared 2 U, fp64 sum, one final rounding: 3 U; margin 1
        assert abs(float(out[1]) - float(conf)) <= 4 * U * abs(float(conf))
        # end to end from the logits in fp64: each logp off by <= tol_lp moves the mean of B of them by
        # <= tol_lp, and the mean of d^2 by <= 2 max|d| tol_lp
        nll_e, conf_e, _, _ = ref64.cls_losses(lp_ref, lab)
        dmax = float((lp_ref - ref64.LOG_HALF_F32).abs().max())
        assert abs(float(out[0]) - float(nll_e)) <= float(tol_row.mean()) + 2 * U * abs(float(nll_e))
        assert abs(float(out[1]) - float(conf_e)) <= 2 * dmax * tol_lp + 4 * U * abs(float(conf_e))
        # sa_log_softmax_bwd on the kernel's own dY and Y: dX = dY - expf(Y) * sum dY
        #   sum: (NC-1) U, expf: 4 U, product: U, difference: U (|dX| <= 2 sum|dY|)
        #   <= (NC + 6) U sum_n |dY|; margin 1
        for dY in (dn, dc):
            dX = ops.log_softmax_bwd(dY, LP)
            torch.cuda.synchronize()
            ref = ref64.log_softmax_bwd(dY.cpu(), lpc)
            rowsum = dY.double().cpu().abs().sum(1, keepdim=True)
            bound = (NC + 7) * U * rowsum
            assert bool(((dX.double().cpu() - ref).abs() <= bound).all())
    return LP


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("B", [1, 2, 3, 10, 31, 32, 33, 64, 65, 256])
def test_log_softmax_and_cls_losses(B, scale):
    check_cls(B, 2, scale)


@pytest.mark.parametrize("B", [21, 22, 43])
def test_log_softmax_and_cls_losses_three_classes(B):
    """B*NC = 63, 66, 129: below, just above and twice past the 64 lanes"""
    check_cls(B, 3, 30.0)


@pytest.mark.parametrize("B", [1, 33, 64])
def test_nll_and_confusion_modules(B):
    from speech_anonymization_amd import losses
    x = cls_logits(B, 2, 1.0)
    lp = ref64.log_softmax(x).float()                   # any fp32 logp will do as the input
    lab = torch.randint(0, 2, (B,), generator=gen(400 + B))
    nll, conf, dn, dc = ref64.cls_losses(lp, lab)
    for mod, args, want, gref in ((losses.NLLLoss(), (lab.to(dev()),), nll, dn),
                                  (losses.ConfusionLoss(), (), conf, dc)):
        for view in (lambda t: t.to(dev()), offset_view):
            p = view(lp).detach().requires_grad_(True)
            loss = mod(p, *args)
            assert abs(float(loss) - float(want)) <= 4 * U * abs(float(want))
            (0.1 * loss).backward()
            # the kernel's gradient (<= 2 roundings), float32(0.1), the product: 4 U; margin 1
            e = (p.grad.double().cpu() - 0.1 * gref).abs() / (0.1 * gref).abs().clamp_min(1e-300)
            assert float(e.max()) <= 5 * U
            ln = mod(view(lp), *args)                   # no-grad path
            assert torch.equal(ln, loss.detach()) and not ln.requires_grad
    # a python list of labels, as the reference's batches carry them
    l2 = losses.NLLLoss()(lp.to(dev()), lab.tolist())
    assert abs(float(l2) - float(nll)) <= 4 * U * abs(float(nll))


# ================================================================================================
# sa_cosine_loss
# ================================================================================================
COS_EPS = 1e-6
DEGENERATE = ["x1_zero", "x2_zero", "both_zero", "tiny_x1", "clamped"]


def cosine_inputs(B, S, D, seed):
    """Unit-direction rows scaled to norms |x1| in [1e-3, 1e3], |x2| in [1e-2, 1e3] (log-uniform).
    The kernel, like torch 1.10, forms |x1|^2 |x2|^2 in fp32: these norms keep it within
    [1e-10, 1e12], far from fp32 overflow / underflow and a factor 1e2 above the clamp at eps^2 =
    1e-12, so the fp64 reference and the kernel take the same branch.  Degenerate rows go to known
    places, the last row (a partial workgroup when B*S % 4 != 0) among them."""
    g = gen(seed)
    rows = B * S
    x1, x2 = torch.randn(rows, D, generator=g, dtype=torch.float64), torch.randn(rows, D, generator=g, dtype=torch.float64)
    x1 = x1 / x1.norm(dim=1, keepdim=True) * 10.0 ** (6.0 * torch.rand(rows, 1, generator=g, dtype=torch.float64) - 3.0)
    x2 = x2 / x2.norm(dim=1, keepdim=True) * 10.0 ** (5.0 * torch.rand(rows, 1, generator=g, dtype=torch.float64) - 2.0)
    where = {}
    if rows >= 6 and D >= 2:
        for name, r in zip(DEGENERATE, [rows - 1, 1, rows // 2, 2, rows - 2]):
            where[name] = r
            u1, u2 = x1[r] / x1[r].norm(), x2[r] / x2[r].norm()
            if name == "x1_zero":
                x1[r] = 0.0
            elif name == "x2_zero":
                x2[r] = 0.0
            elif name == "both_zero":
                x1[r] = 0.0; x2[r] = 0.0
            elif name == "tiny_x1":                     # 1e-7 * 100 = 1e-5 > eps: NOT clamped in 1.10
                x1[r] = 1e-7 * u1; x2[r] = 100.0 * u2
            else:                                       # 1e-4 * 1e-4 = 1e-8 < eps: clamped
                x1[r] = 1e-4 * u1; x2[r] = 1e-4 * u2
    return x1.float().reshape(B, S, D), x2.float().reshape(B, S, D), where


def cosine_tolerances(D):
    """Derived, not measured.  A lane accumulates ceil(D/64) fma steps and the wave reduction adds
    log2(64) = 6 levels, so each of dot, |x1|^2, |x2|^2 carries gam = (6 + ceil(D/64)) U relative to
    the sum of the magnitudes of its terms (<= |x1||x2| for the dot product).
      cos = dot / sqrt(max(na nb, eps^2)): gam (dot) + |cos| (gam + 2.5 U) (na nb: 2 gam + U, halved
            by the sqrt; sqrt; divide) + 2 U (1 - cos <= 2)             -> 2 gam + 4.5 U, absolute;
            + 3 U where the value is read back through 1 - (1 - (1 - cos))    -> 2 gam + 8 U
      dx1 = -(1/S) (x2 inv - cos x1 / na), inv = 1 / sqrt(..): the first term carries gam + 3.5 U
            relative; the second the absolute error of cos before the 1 - cos (2 gam + 2.5 U), gam
            (na) and 2 U (product, divide): 3 gam + 4.5 U; the difference, -1/S and the product by
            it: 3 U                                                         -> 3 gam + 8 U < 4 gam + 10 U
    measured against the row's scale (1/S)(|x2|_inf / den + |x1|_inf / na), the size of the two terms
    (clamped rows: the first only): the gradient is their difference and may cancel (exactly so at
    D = 1), and the absolute error of cos does not shrink with |cos|."""
    gam = (6 + -(-D // 64)) * U
    return 2 * gam + 8 * U, 4 * gam + 10 * U


def check_cosine_rows(x1, x2, S, rowloss, dx1, where, tag, extra=0.0):
    """per row: the worst row decides, so that one wrong row cannot hide among thousands"""
    D = x1.shape[-1]
    a, b = x1.reshape(-1, D), x2.reshape(-1, D)
    _, row_ref, g_ref = ref64.cosine_loss(a[:, None, :], b[:, None, :], COS_EPS)   # S = 1 per row
    row_ref, g_ref = row_ref[:, 0], g_ref[:, 0] / S
    cos, na, nb, clamped = ref64.cosine_rows(a, b, COS_EPS)
    tol_v, tol_g = cosine_tolerances(D)
    ev = (rowloss.double().cpu().reshape(-1) - row_ref).abs()
    print(f"cosine {tag}: worst row value err {float(ev.max()) / U:.2f} U at row {int(ev.argmax())} (bound {tol_v / U:.0f} U)")
    assert float(ev.max()) <= tol_v
    for name, r in where.items():
        assert bool(clamped[r]) == (name != "tiny_x1"), name
    if dx1 is None:
        return
    den = torch.sqrt(torch.clamp_min(na * nb, ref64.f32_eps(COS_EPS) ** 2))
    scale = b.double().abs().max(1)[0] / den
    scale = scale + torch.where(clamped, torch.zeros_like(na),
                                a.double().abs().max(1)[0] / na.clamp_min(1e-300))
    scale = scale / S
    err = (dx1.double().cpu().reshape(-1, D) - g_ref).abs().max(1)[0]
    zero = scale == 0                                   # x2 row zero: the gradient is exactly 0
    assert float(err[zero].sum()) == 0.0
    rel = err[~zero] / scale[~zero]
    print(f"  worst row gradient err {float(rel.max()) / U:.2f} U (bound {tol_g / U:.0f} U)")
    assert float(rel.max()) <= tol_g + extra


# B*S % 4: 1, 2, 1, 1, 1, 0;  D < 64, = 63 / 64 / 65, the recogniser's (32, 252, 768)
@pytest.mark.parametrize("B,S,D", [(1, 1, 1), (2, 3, 5), (3, 7, 63), (3, 7, 64), (3, 7, 65), (32, 252, 768)])
def test_cosine_loss_shapes(B, S, D):
    from speech_anonymization_amd import ops
    x1, x2, where = cosine_inputs(B, S, D, seed=500 + D + S)
    assert (B, S, D) == (1, 1, 1) or len(where) == 5
    want, _, _ = ref64.cosine_loss(x1, x2, COS_EPS)
    x1d, x2d = x1.to(dev()), x2.to(dev())
    loss, dx1 = ops.cosine_loss(x1d, x2d, want_grad=True)
    loss2, none = ops.cosine_loss(x1d, x2d, want_grad=False)
    rows = 1.0 - ops.cosine_rows(x1d.reshape(-1, D), x2d.reshape(-1, D))
    torch.cuda.synchronize()
    assert none is None and torch.equal(loss, loss2)
    check_cosine_rows(x1, x2, S, rows, dx1, where, f"({B},{S},{D})")
    # loss = fp64 sum of the rows / S, one rounding
    tol_v, _ = cosine_tolerances(D)
    assert abs(float(loss) - float(want)) <= B * tol_v + U * abs(float(want))


def test_cosine_rows_and_module():
    """ops.cosine_rows at (5, 768) (the S = 1 use of the evaluation hook), CosineSimilarityLoss with
    an upstream factor, the no-grad path, bf16 / non-contiguous / offset inputs."""
    from speech_anonymization_amd import losses, ops
    x1, x2, _ = cosine_inputs(5, 1, 768, seed=601)
    cs = ops.cosine_rows(x1[:, 0].to(dev()), x2[:, 0].to(dev()))
    torch.cuda.synchronize()
    check_cosine_rows(x1, x2, 1, 1.0 - cs, None, {}, "rows (5,768)")
    B, S, D = 3, 7, 65
    x1, x2, where = cosine_inputs(B, S, D, seed=602)
    want, _, gref = ref64.cosine_loss(x1, x2, COS_EPS)
    mod = losses.CosineSimilarityLoss()
    tol_v, _ = cosine_tolerances(D)
    for view in (lambda t: t.to(dev()), offset_view,
                 lambda t: t.transpose(0, 1).contiguous().to(dev()).transpose(0, 1)):
        p = view(x1).detach().requires_grad_(True)
        loss = mod(p, view(x2))
        assert abs(float(loss) - float(want)) <= B * tol_v + U * abs(float(want))
        (0.1 * loss).backward()
        # 0.1 * gradient adds float32(0.1) and the product (2 U) to the kernel's own bound
        rl = 1.0 - ops.cosine_rows(view(x1).reshape(-1, D), view(x2).reshape(-1, D))
        check_cosine_rows(x1, x2, S, rl, p.grad.double() / float(np.float32(0.1)), where, "module", extra=2 * U)
        ln = mod(view(x1), view(x2))
        assert torch.equal(ln, loss.detach()) and not ln.requires_grad
    # bf16 inputs are widened exactly
    xb1, xb2 = x1.to(torch.bfloat16), x2.to(torch.bfloat16)
    wb, _, _ = ref64.cosine_loss(xb1.float(), xb2.float(), COS_EPS)
    lb = mod(xb1.to(dev()), xb2.to(dev()))
    assert abs(float(lb) - float(wb)) <= B * tol_v + U * abs(float(wb))


# ================================================================================================
# sa_cluster_mi
# ================================================================================================
def mi_pool(N, D, ncls, seed, dup=False):
    """Gaussian pool X = randn(N, D) + 0.3 y with balanced classes y = i % ncls"""
    g = gen(seed)
    y = torch.arange(N) % ncls
    X = torch.randn(N, D, generator=g) + 0.3 * y[:, None].float()
    if dup:                                             # exact duplicates inside a class: ties in d <= anchor
        X[N // 2:] = X[:N - N // 2]
        y[N // 2:] = y[:N - N // 2]
    return X, y


# (pool N, D, n, k, classes, duplicated rows)
MI_SETS = [
    (8, 128, 4, 3, 2, False),        # 2 + 2 members: every anchor is 10e6, m = n - 1
    (64, 256, 8, 3, 2, False),
    (64, 2, 32, 3, 2, False), (64, 256, 32, 3, 2, False), (64, 1000, 32, 3, 2, False),
    (64, 128, 32, 3, 2, True),
    (128, 128, 64, 3, 2, False),     # n*n = 4096 = 16 x 256: the last full round of the pair loop
    (320, 256, 66, 1, 2, False),
    (297, 256, 99, 3, 3, False),
    (320, 128, 160, 3, 2, False), (320, 256, 160, 3, 2, False), (320, 1000, 160, 3, 2, False),
    (320, 256, 160, 8, 2, False),
]


def mi_reference(X, y, idx, ncls, k):
    """ref64 value and admissible interval, with the two conditions that keep the comparison a test:
    at least half of the sets are compared exactly, no interval is wider than 0.03 bit.
    tau = 8 x (fp32 CPU evaluation of the distance formula vs fp64) on this pool; the 8 covers the
    kernel's serial fma order against the blocked order of the CPU matmul."""
    tau = ref64.distance_tau(X, margin=8.0)
    mi, lo, hi = ref64.cluster_mi(X, y, idx, ncls=ncls, k=k, tau=tau)
    width = hi - lo
    assert (width == 0).sum() * 2 >= len(width), f"only {(width == 0).sum()} of {len(width)} sets exact"
    assert width.max() <= 0.03, f"widest interval {width.max():.4f} bit"
    return mi, lo, hi, tau


def assert_mi(got, lo, hi, tag, tau):
    got = np.asarray(got, dtype=np.float64)
    out = np.maximum(lo - got, got - hi)
    print(f"mi {tag}: tau {tau:.2e}, {int(((hi - lo) > 0).sum())} of {len(lo)} sets undecided, widest "
          f"{(hi - lo).max():.4f} bit, worst distance to the interval {out.max():.2e}")
    # 1e-5: the kernel's fp64 digamma series (< 1e-10) and one fp32 rounding of a value below 4 bits
    assert out.max() <= 1e-5


@pytest.mark.parametrize("N,D,n,k,ncls,dup", MI_SETS)
def test_cluster_mi_resampled_sets(N, D, n, k, ncls, dup):
    """100 class-balanced index sets drawn as MILoss draws them, through ops.cluster_mi and through
    MILoss.forward (numpy seeded before it, so the draws can be replayed for the reference)."""
    from speech_anonymization_amd import losses, ops
    X, y = mi_pool(N, D, ncls, seed=700 + N + D + n + k, dup=dup)
    groups = y.tolist()
    np.random.seed(n * 10 + k)
    idx = losses.MILoss.sample_index_sets(groups, n // ncls, 100)
    assert idx.shape == (100, n)
    mi, lo, hi, tau = mi_reference(X, y, idx, ncls, k)
    Xd, yd = X.to(dev()), y.to(dev())
    got = ops.cluster_mi(Xd, yd, torch.from_numpy(idx).to(dev()), ncls=ncls, k=k)
    np.random.seed(n * 10 + k)
    lst = losses.MILoss(n_iterations=100, k=k)(Xd.reshape(N, 1, D), yd, groups, n // ncls, n_classes=ncls)
    torch.cuda.synchronize()
    assert len(lst) == 100
    assert_mi(got.cpu().numpy(), lo, hi, f"N={N} D={D} n={n} k={k}", tau)
    assert torch.equal(torch.stack(lst), got)
    if n == 4:                                          # no same-class set of k + 1: m = n - 1 everywhere
        c = math.log(2.0)
        dg = lambda v: float(torch.digamma(torch.tensor(float(v), dtype=torch.float64)))
        assert np.allclose(mi, (dg(4) - dg(2) + dg(3) - dg(3)) / c, atol=1e-12)


@pytest.mark.parametrize("case", ["n160", "n4", "imbalanced", "duplicates", "three_classes", "k_plus_1"])
def test_cluster_mi_whole_batch(case):
    """idx=None: one estimate over rows 0..n-1"""
    from speech_anonymization_amd import ops
    k, ncls = 3, 2
    if case == "n160":
        # a single set has to be an exact one: of the pool seeds 810..821 eight give an interval of
        # zero width (reference side only), 810 is the first
        X, y = mi_pool(160, 256, 2, seed=810)
    elif case == "n4":
        X, y = mi_pool(4, 128, 2, seed=802)
    elif case == "imbalanced":                          # 3 + 29: class 0 has fewer than k + 1 members
        X, _ = mi_pool(32, 128, 2, seed=803)
        y = torch.tensor([0] * 3 + [1] * 29)
        X = X + 0.3 * y[:, None].float()
    elif case == "duplicates":
        X, y = mi_pool(32, 40, 2, seed=804, dup=True)
    elif case == "three_classes":
        X, y = mi_pool(99, 128, 3, seed=805)
        ncls = 3
    else:                                               # n = k + 1 = 9 at the largest k
        X, y = mi_pool(9, 128, 2, seed=806)
        k = 8
    mi, lo, hi, tau = mi_reference(X, y, None, ncls, k)
    got = ops.cluster_mi(X.to(dev()), y.to(dev()), ncls=ncls, k=k)
    torch.cuda.synchronize()
    assert got.shape == (1,)
    assert_mi(got.cpu().numpy(), lo, hi, case, tau)


def test_cluster_mi_refusals():
    """n > 160 (LDS), k outside 1..8 and n <= k return -22 before any launch; L.check raises"""
    from speech_anonymization_amd import ops
    from speech_anonymization_amd._lib import SaHipError
    X, y = mi_pool(161, 16, 2, seed=901)
    Xd, yd = X.to(dev()), y.to(dev())
    for Xc, yc, k in ((Xd, yd, 3), (Xd[:32], yd[:32], 9), (Xd[:32], yd[:32], 0), (Xd[:3], yd[:3], 3),
                      (Xd[:8], yd[:8], 8)):
        with pytest.raises(SaHipError):
            ops.cluster_mi(Xc.contiguous(), yc.contiguous(), k=k)
    torch.cuda.synchronize()
    ok = ops.cluster_mi(Xd[:160].contiguous(), yd[:160].contiguous(), k=8)      # the limits themselves pass
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ok).all())


# ================================================================================================
# sa_pool_fwd / _gather / _fin / _bwd
# ================================================================================================
# sa_pool_nseg: B <= 16 -> 8, 32 -> 4, 64 -> 2, >= 128 -> 1.  L < 128: one k-block, every segment but
# the first is empty; 127 / 128 / 129 straddle the block; L = 2 is the smallest accepted.
POOL_SHAPES = [(1, 2, 8), (1, 127, 8), (3, 128, 8), (3, 129, 8), (32, 333, 4), (64, 333, 2), (130, 200, 1),
               (32, 20146, 4)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Ln,nseg", POOL_SHAPES)
def test_statistics_pooling_shapes(dt, B, Ln, nseg):
    """Forward (with and without the noise term), backward and the fused BatchNorm-backward
    statistics against ref64.stat_pool, with the limits of test_statistics_pooling_reshape_quirk
    (rel-MSE 1e-9; 2e-5 for the bf16 gradient: one bf16 rounding, 2^-9 relative, squared, is 3.8e-6).
    Inputs are |randn| * scale + shift, never constant over a pooled column: at zero variance
    torch's sqrt backward is non-finite where the kernel returns 0 -- a known, separate difference
    that is not tested here."""
    from speech_anonymization_amd import _lib as L, ops
    assert L.load().sa_pool_nseg(B) == nseg
    Cc = 128
    r = torch.randn(B, Cc, Ln, generator=gen(41 + B + Ln)).abs().to(dt).float()
    sc = 1 + 0.1 * torch.randn(Cc, generator=gen(42))
    sh = 0.1 * torch.randn(Cc, generator=gen(43))
    gp = torch.randn(B, 256, generator=gen(44))
    noise = torch.rand(B, 128, generator=gen(47))
    xbn = r.double() * sc.double()[None, :, None] + sh.double()[None, :, None]
    pooled, _, std = ref64.stat_pool(xbn)
    assert float(std.min()) > 1e-3
    pooled_n, _, _ = ref64.stat_pool(xbn, noise=noise)
    gx = ref64.stat_pool_bwd(xbn, gp)
    del xbn
    rd = r.permute(0, 2, 1).contiguous().to(dev(), dt)
    scd, shd, gpd = sc.to(dev()), sh.to(dev()), gp.to(dev())
    pd, mean, sd = ops.pool_fwd(rd, scd, shd)
    g = ops.pool_bwd(rd, scd, shd, gpd, mean, sd)
    pn, _, _ = ops.pool_fwd(rd, scd, shd, noise=noise.to(dev()))
    torch.cuda.synchronize()
    e_p, e_n = rel_mse(pd, pooled), rel_mse(pn, pooled_n)
    e_g = rel_mse(g.float().cpu().permute(0, 2, 1), gx)
    print(f"pool {dt} B={B} L={Ln}: pooled {e_p:.2e} noise {e_n:.2e} grad {e_g:.2e}")
    assert e_p < 1e-9 and e_n < 1e-9
    assert e_g < (1e-9 if dt == torch.float32 else 2e-5)
    # the halves separately, so that a wrong std cannot hide behind a larger mean
    assert rel_mse(pd[:, :128], pooled[:, :128]) < 1e-9 and rel_mse(pd[:, 128:], pooled[:, 128:]) < 1e-9
    # fused BatchNorm-backward statistics of the written gradient == a separate sa_ew_stats pass
    bm = (0.1 * torch.randn(Cc, generator=gen(45))).to(dev())
    br = (1 + 0.1 * torch.randn(Cc, generator=gen(46))).abs().to(dev())
    g2, st = ops.pool_bwd(rd, scd, shd, gpd, mean, sd, bn=(bm, br))
    st_ref = ops.ew("stats", g, rd, Cc, mean=bm, rstd=br, per_c=True)
    torch.cuda.synchronize()
    assert torch.equal(g2, g)
    a, b_ = ops.sum_partials(st, 1).cpu(), ops.sum_partials(st_ref, 1).cpu()
    assert rel_mse(a, b_) < (1e-10 if dt == torch.float32 else 1e-6)
    if B * Ln <= 50000:                                 # and against fp64 sums of the stored gradient
        gd, xd = g.double().cpu(), rd.double().cpu()
        xh = (xd - bm.double().cpu()) * br.double().cpu()
        ref = torch.stack([gd.sum((0, 1)), (gd * xh).sum((0, 1))], dim=-1)
        assert rel_mse(a.reshape(Cc, 2), ref) < (1e-10 if dt == torch.float32 else 1e-6)
