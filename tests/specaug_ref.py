"""fp64 restatement of a SpecAugment plan (speech_anonymization_amd.specaug), shared by
tests/test_specaug_cpu.py and tests/test_specaug_gpu.py.  It takes the plan's own int32 indices and fp32 weights cast
up, so only the arithmetic of the kernels is compared, and the semantics are written out a second time: warp,
frequency masks filled with the mean of the warped tensor, time masks filled with the mean after the frequency masks."""
import types

import torch

EPS = 2.0 ** -24


def warp64(x, plan):
    """x [B, T, F] -> (y [B, T, F] fp64, sw [T] fp64: sum_k |w[o][k]|, exact [T] bool: rows with weights 0, 1, 0, 0)"""
    x = x.detach().double().cpu()
    w = plan.wt.double()
    y = torch.zeros_like(x)
    for k in range(4):
        idx = torch.minimum(torch.maximum(plan.base.long() - 1 + k, plan.lo.long()), plan.hi.long())
        y += w[:, k].view(1, -1, 1) * x[:, idx]
    exact = (plan.wt == torch.tensor([0.0, 1.0, 0.0, 0.0])).all(1)
    return y, w.abs().sum(1), exact


def warp_bar(x, plan, sw):
    """per element [B, T, 1]: 8 * 2^-24 * sum_k |w[o][k]| * max |x_b| -- four products, three adds, a weight
    already rounded"""
    amax = x.detach().double().cpu().abs().amax((1, 2))
    return 8 * EPS * sw.view(1, -1, 1) * amax.view(-1, 1, 1)


def restate(x, plan):
    """-> warp [B, T, F] fp64, bar [B, T, 1], exact [T], fm [B, F], tm [B, T], val_f, val_t (fp64), out [B, T, F]
    fp64 (the whole augmentation), val_bar (the bar of a mean of warped values)"""
    y, sw, exact = warp64(x, plan)
    bar = warp_bar(x, plan, sw)
    fm, tm = plan.masks()
    out = y.clone()
    val_f = 0.0 if plan.zero else float(out.mean())
    out[fm[:, None, :].expand_as(out)] = val_f
    val_t = 0.0 if plan.zero else float(out.mean())
    out[tm[:, :, None].expand_as(out)] = val_t
    return types.SimpleNamespace(warp=y, bar=bar, exact=exact, fm=fm, tm=tm, val_f=val_f, val_t=val_t, out=out,
                                 val_bar=float(bar.max()))


def check_output(got, x, plan, tag=""):
    """got: the kernels' output for input x (both CPU).  Asserts every property the definition gives and returns
    the restatement.  Prints each figure first."""
    r = restate(x, plan)
    got = got.detach().cpu()
    assert got.shape == x.shape and got.dtype == torch.float32
    cell_t = r.tm[:, :, None].expand_as(got)
    cell_f = r.fm[:, None, :].expand_as(got) & ~cell_t
    free = ~(cell_t | cell_f)
    err = (got.double() - r.warp).abs()
    worst = float((err / r.bar.clamp_min(1e-300))[free].max()) if bool(free.any()) else 0.0
    rows = r.exact.view(1, -1, 1).expand_as(got) & free
    idx = torch.minimum(torch.maximum(plan.base.long(), plan.lo.long()), plan.hi.long())
    src = x.detach().cpu()[:, idx]
    n_exact_bad = int((got[rows] != src[rows]).sum())
    vf = got[cell_f].unique() if bool(cell_f.any()) else torch.empty(0)
    vt = got[cell_t].unique() if bool(cell_t.any()) else torch.empty(0)
    print(f"{tag}: B,T,F={tuple(x.shape)} c={plan.c} w={plan.w} free {int(free.sum())} worst err/bar {worst:.4f} "
          f"exact rows {int(r.exact.sum())} (mismatches {n_exact_bad}) freq cells {int(cell_f.sum())} values "
          f"{vf.tolist()} (ref {r.val_f:.9g}) time cells {int(cell_t.sum())} values {vt.tolist()} (ref {r.val_t:.9g}) "
          f"val bar {r.val_bar:.3e}")
    assert bool((err <= r.bar)[free].all()), worst
    assert n_exact_bad == 0
    for v, ref in ((vf, r.val_f), (vt, r.val_t)):
        assert v.numel() <= 1, "filled cells are not bit-equal to one value"
        if v.numel():
            if plan.zero:
                assert float(v) == 0.0
            else:
                assert abs(float(v) - ref) <= r.val_bar + 2 * EPS * abs(ref), (float(v), ref)
    return r
