"""x-vector gender classifier on libsa_hip.so (in the training graph: 8f-1): drop-in for the
``embedding_model`` / ``classifier`` pair of speechbrain_configs/evaluator_inference.yaml:34-48
(``speechbrain.lobes.models.Xvector.Xvector`` / ``.Classifier``, restated in the reference at
models/external_gender_classifiers.py:24-183).  Same constructor defaults as that config, same
parameter names (``blocks.0.conv.weight`` ... ``blocks.16.w.weight``; ``norm.norm.weight``,
``DNN.block_0.linear.w.weight``, ``out.w.weight`` as in the reference's classifier.ckpt), eval
mode (BatchNorm running statistics).  ``classify_batch_feats(feats, lens)`` is the call the
reference's fork adds (speechbrain_convae_train.py:139,146): returns (log_probs, score, index).

``EncoderClassifier.forward(feats)`` is the same computation INSIDE the training graph
(models/EndToEnd.py:57-61,81: ``self.sex_classifier(input)`` on the reconstructed features, the
classifier pretrained and frozen): differentiable with respect to the features only
(sa_tdnn_bwd_input / sa_tdnn_fold / sa_time_pool_bwd / sa_leaky_affine_bwd); its parameters never
receive gradients.

``train_log_probs`` is the TRAIN mode of gender_classifier_train.py (_XvTrainFn).  All kernels are in
csrc/sa_xvector.hip; the dense layers, softmax and finalisers in sa_head.hip / sa_elementwise.hip.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from . import ops


class _Conv(nn.Module):
    def __init__(self, cin, cout, k, d):
        super().__init__()
        self.kernel_size, self.dilation = k, d
        self.conv = nn.Conv1d(cin, cout, k, dilation=d)


class _BN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.norm = nn.BatchNorm1d(c)

    def affine(self):
        n = self.norm
        return ops.fin_bn_eval(n.num_features, n.weight, n.bias, n.running_mean, n.running_var, n.eps)


class _Lin(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.w = nn.Linear(cin, cout)


class _Marker(nn.Module):
    pass


def _packed(conv):
    """split-bf16 operand image of the (frozen, eval-mode) Conv1d weight, output channels zero-padded
    to a multiple of 128; rebuilt when the parameter changes."""
    w = conv.conv.weight
    key = (w.data_ptr(), w._version, str(w.device))
    if getattr(conv, "_img_key", None) != key:
        Cout, Cin, K = w.shape
        npad = -(-Cout // 128) * 128
        wpad = w.detach()
        if npad != Cout:
            wpad = torch.cat([wpad, torch.zeros(npad - Cout, Cin, K, dtype=w.dtype, device=w.device)])
        conv._img = ops.pack_weights(wpad.contiguous().float(), "conv_fwd", torch.float32, L.BF16X3)
        conv._img_key, conv._npad = key, npad
    return conv._img, conv._npad


def _packed_dgrad(conv):
    """the same weight as a data-gradient operand: reduction over the block's output channels
    (zero-padded to a multiple of 16), produced = its input channels (zero-padded to 128)."""
    w = conv.conv.weight
    key = (w.data_ptr(), w._version, str(w.device))
    if getattr(conv, "_dimg_key", None) != key:
        Cout, Cin, K = w.shape
        cred, npad = -(-Cout // 16) * 16, -(-Cin // 128) * 128
        wpad = torch.zeros(cred, npad, K, dtype=torch.float32, device=w.device)
        wpad[:Cout, :Cin] = w.detach().float()
        conv._dimg = ops.pack_weights(wpad, "conv_dgrad", torch.float32, L.BF16X3)
        conv._dimg_key, conv._dgeom = key, (cred, npad)
    return conv._dimg, conv._dgeom


def _linear(v, lin):
    return ops.dense(v, lin.weight, lin.bias, lin.out_features, lin.in_features)


def _linear_T(g, lin):
    """d loss / d input of _linear"""
    return ops.dense(g, lin.weight, None, lin.in_features, lin.out_features, transpose_w=True)


def _leaky(x, s=None, t=None, slope=0.01):
    """LeakyReLU, then the per-channel affine s*v + t where given, on [M, C]"""
    y = torch.empty_like(x)
    L.check(L.load().sa_leaky_affine(L.ptr(x), L.ptr(s), L.ptr(t), C.c_float(slope), x.shape[0], x.shape[1],
                                     L.ptr(y), L.stream()), "sa_leaky_affine")
    return y


def _leaky_bwd(dy, x, s, slope=0.01):
    dx = torch.empty_like(x)
    L.check(L.load().sa_leaky_affine_bwd(L.ptr(dy), L.ptr(x), L.ptr(s), C.c_float(slope), x.shape[0], x.shape[1],
                                         L.ptr(dx), L.stream()), "sa_leaky_affine_bwd")
    return dx


def _lens(lens, device):
    return None if lens is None else lens.to(device).float().contiguous()


def _time_pool(h, lens_d, noise):
    B, T, Cc = h.shape
    pooled = torch.empty(B, 2 * Cc, dtype=torch.float32, device=h.device)
    L.check(L.load().sa_time_pool(L.ptr(h), L.ptr(lens_d), L.ptr(noise), B, T, Cc, C.c_float(1e-5), L.ptr(pooled),
                                  L.stream()), "sa_time_pool")
    return pooled


def _time_pool_bwd(h, lens_d, g, pooled0):
    B, T, Cc = h.shape
    gh = torch.empty_like(h)
    L.check(L.load().sa_time_pool_bwd(L.ptr(h), L.ptr(lens_d), L.ptr(g), L.ptr(pooled0), B, T, Cc, C.c_float(1e-5),
                                      L.ptr(gh), L.stream()), "sa_time_pool_bwd")
    return gh


def _dgrad(g, conv, launch):
    """data gradient of one TDNN block from g [B, T, Cy]: the packed data-gradient image, the
    extended buffer [B, T + 2*pad, Cin], launch(lib, img, dxe, cred, npad), the reflect adjoint."""
    lib = L.load()
    B, T, _ = g.shape
    Cin, K, dil = conv.conv.in_channels, conv.kernel_size, conv.dilation
    img, (cred, npad) = _packed_dgrad(conv)
    pad = dil * (K - 1) // 2
    dxe = torch.empty(B, T + 2 * pad, Cin, dtype=torch.float32, device=g.device)
    launch(lib, img, dxe, cred, npad)
    if pad == 0:
        return dxe
    dx = torch.empty(B, T, Cin, dtype=torch.float32, device=g.device)
    L.check(lib.sa_tdnn_fold(L.ptr(dxe), L.ptr(dx), B, T, Cin, pad, L.stream()), "sa_tdnn_fold")
    return dx


def _tdnn_bwd(dy, mask, conv, bn, slope=0.01):
    """d loss / d x of one frozen TDNN block from d loss / d y and the forward's LeakyReLU mask."""
    B, T, Cy = mask.shape
    s = bn.affine()[2]
    return _dgrad(dy, conv, lambda lib, img, dxe, cred, npad: L.check(
        lib.sa_tdnn_bwd_input(L.ptr(dy), L.ptr(mask), L.ptr(s), L.ptr(img), L.ptr(dxe), B, T, Cy, cred,
                              conv.conv.in_channels, npad, conv.kernel_size, conv.dilation, C.c_float(slope),
                              L.stream()), "sa_tdnn_bwd_input"))


def _tdnn(x, conv, bn, slope=0.01, want_mask=False):
    lib = L.load()
    B, T, Cin = x.shape
    Cout = conv.conv.out_channels
    _, _, s, t = bn.affine()
    img, npad = _packed(conv)
    y = torch.empty(B, T, Cout, dtype=torch.float32, device=x.device)
    mask = torch.empty(B, T, Cout, dtype=torch.uint8, device=x.device) if want_mask else None
    L.check(lib.sa_tdnn_fwd(L.ptr(x), L.ptr(img), L.ptr(conv.conv.bias), L.ptr(s), L.ptr(t),
                            L.ptr(y), B, T, Cin, Cout, npad, conv.kernel_size, conv.dilation,
                            C.c_float(slope), L.ptr(mask), L.stream()), "sa_tdnn_fwd")
    return (y, mask) if want_mask else y


def _frozen_embed(xv, feats, lens, want_masks):
    """the eval-mode Xvector: (embedding [B, emb], masks, h, lens_d, pooled0).  Without masks (the
    no-grad path) sa_time_pool adds the pooling noise and pooled0 is None; with them (in the
    graph) it pools without noise and the noise is added afterwards, because the backward needs
    the noise-free pooled0."""
    h, masks = feats.contiguous().float(), []
    for conv, bn in xv.tdnn():
        h = _tdnn(h, conv, bn, want_mask=want_masks)
        if want_masks:
            h, m = h
            masks.append(m)
    B, _, Cc = h.shape
    noise = ops.pooling_noise(xv.pooling_noise, B, Cc, h.device)
    lens_d = _lens(lens, h.device)
    if not want_masks:
        return _linear(_time_pool(h, lens_d, noise), xv.blocks[-1].w), None, None, None, None
    pooled = pooled0 = _time_pool(h, lens_d, None)
    if noise is not None:
        pooled = pooled0.clone()
        pooled[:, :Cc] += 1e-5 * ((1.0 - 9.0) * noise + 9.0)
    return _linear(pooled, xv.blocks[-1].w), masks, h, lens_d, pooled0


def _frozen_head(cl, emb):
    """the eval-mode Classifier on emb [B, emb]: (log-probabilities [B, classes], h1)"""
    blk = cl.DNN["block_0"]
    h1 = _linear(_leaky(emb, *cl.norm.affine()[2:]), blk.linear.w)
    return ops.log_softmax(_linear(_leaky(h1, *blk.norm.affine()[2:]), cl.out.w)), h1


class Xvector(nn.Module):
    def __init__(self, in_channels=80, lin_neurons=128, tdnn_channels=(512, 512, 512, 512, 1500),
                 tdnn_kernel_sizes=(5, 3, 3, 1, 1), tdnn_dilations=(1, 2, 3, 1, 1), pooling_noise=True,
                 **_ignored):
        super().__init__()
        self.blocks = nn.ModuleList()
        for c, k, d in zip(tdnn_channels, tdnn_kernel_sizes, tdnn_dilations):
            self.blocks.extend([_Conv(in_channels, c, k, d), _Marker(), _BN(c)])
            in_channels = c
        self.blocks.append(_Marker())                       # StatisticsPooling
        self.blocks.append(_Lin(in_channels * 2, lin_neurons))
        self.pooling_noise = pooling_noise
        self.eval()

    def tdnn(self):
        """the (conv, bn) pairs of the TDNN blocks, first to last"""
        return [(self.blocks[i], self.blocks[i + 2]) for i in range(0, len(self.blocks) - 2, 3)]

    @torch.no_grad()
    def forward(self, x, lens=None):
        return _frozen_embed(self, x, lens, False)[0].unsqueeze(1)      # [B, 1, emb]


class _Block(nn.Module):
    def __init__(self, n_in, n_out):
        super().__init__()
        self.linear, self.act, self.norm = _Lin(n_in, n_out), _Marker(), _BN(n_out)


class Classifier(nn.Module):
    def __init__(self, input_shape=None, lin_blocks=1, lin_neurons=128, out_neurons=2, **_ignored):
        super().__init__()
        emb = input_shape[-1] if input_shape else 128
        assert lin_blocks == 1
        self.act = _Marker()
        self.norm = _BN(emb)
        self.DNN = nn.ModuleDict({"block_0": _Block(emb, lin_neurons)})
        self.out = _Lin(lin_neurons, out_neurons)
        self.eval()

    @torch.no_grad()
    def forward(self, x):
        return _frozen_head(self, x.reshape(x.shape[0], -1).contiguous().float())[0].unsqueeze(1)  # [B, 1, classes]


class _XvFn(torch.autograd.Function):
    """log-probabilities of the frozen x-vector classifier as a function of the features."""

    @staticmethod
    def forward(ctx, enc, feats, lens):
        emb, masks, h, lens_d, pooled0 = _frozen_embed(enc.embedding_model, feats.detach(), lens, True)
        logp, h1 = _frozen_head(enc.classifier, emb)
        ctx.enc, ctx.saved = enc, (masks, h, lens_d, pooled0, emb, h1, logp)
        return logp

    @staticmethod
    def backward(ctx, d_logp):
        xv, cl = ctx.enc.embedding_model, ctx.enc.classifier
        masks, h, lens_d, pooled0, emb, h1, logp = ctx.saved
        blk = cl.DNN["block_0"]
        g = _linear_T(ops.log_softmax_bwd(d_logp.contiguous().float(), logp), cl.out.w)
        g = _linear_T(_leaky_bwd(g, h1, blk.norm.affine()[2]), blk.linear.w)
        g = _linear_T(_leaky_bwd(g, emb, cl.norm.affine()[2]), xv.blocks[-1].w)
        gh = _time_pool_bwd(h, lens_d, g, pooled0)
        for (conv, bn), mask in zip(reversed(xv.tdnn()), reversed(masks)):
            gh = _tdnn_bwd(gh, mask, conv, bn)
        ctx.saved = None
        return None, gh, None


def _colsums(G, H=None, mean=None, rstd=None, coef=None, out=None, slope=0.01):
    """fp64 per-channel partial rows [R, N, 2] of sa_xv_colsums over G [M, N] (see include/sa_hip.h)."""
    M, N = G.shape
    nchunk = min(64, -(-M // 256))
    rows_per = -(-M // nchunk)
    part = torch.empty(-(-M // rows_per), N, 2, dtype=torch.float64, device=G.device)
    c1, c2, c3 = coef if coef is not None else (None, None, None)
    L.check(L.load().sa_xv_colsums(L.ptr(G), L.ptr(H), L.ptr(mean), L.ptr(rstd), L.ptr(c1), L.ptr(c2), L.ptr(c3),
                                   C.c_float(slope), L.ptr(out), M, N, rows_per, L.ptr(part), L.stream()),
            "sa_xv_colsums")
    return part


def _bn_train_stats(part, norm, count):
    """fp64 finaliser of the batch statistics: (mean, rstd, scale, shift); updates the running
    statistics (momentum, unbiased variance) and num_batches_tracked like torch's BatchNorm."""
    f = ops.fin_bn_fwd(part, norm.num_features, float(count), norm.weight, norm.bias, norm.running_mean,
                       norm.running_var, norm.eps, norm.momentum)
    norm.num_batches_tracked.add_(1)
    return f


def _bn_leaky_bwd(dy, z, norm, f, count, dgamma, dbeta, dpre):
    """BatchNorm(train) then LeakyReLU backward on z = leaky(pre) [M, N]: the BatchNorm sums and the
    folded coefficients (fp64), then dpre = leak'(z) * (c1*dy + c2*z + c3); returns the fp64
    partial rows of sum dpre (the bias gradient of the layer before)."""
    mean, rstd = f[0], f[1]
    sums = _colsums(dy, z, mean, rstd)
    coef = ops.fin_norm_bwd(sums, None, norm.num_features, norm.num_features, float(count), norm.weight, mean,
                            rstd, dgamma=dgamma, dbeta=dbeta)
    return _colsums(dy, z, coef=coef, out=dpre)


def _fin_bias(part, db):
    return ops.fin_bias(part, part.shape[0], part.shape[1], db)


def _tdnn_train(x, s_in, t_in, conv, slope=0.01):
    """z = leaky(conv(s_in*x + t_in) + bias) and the fp32 (sum z, sum z^2) tile partials."""
    lib = L.load()
    B, T, Cin = x.shape
    Cout = conv.conv.out_channels
    _stale(conv)
    img, npad = _packed(conv)
    z = torch.empty(B, T, Cout, dtype=torch.float32, device=x.device)
    part = torch.empty(1, B * lib.sa_xv_tdnn_ntiles(T), 2 * Cout, dtype=torch.float32, device=x.device)
    L.check(lib.sa_xv_tdnn_fwd_train(L.ptr(x), L.ptr(s_in), L.ptr(t_in), L.ptr(img), L.ptr(conv.conv.bias),
                                     L.ptr(z), L.ptr(part), B, T, Cin, Cout, npad, conv.kernel_size, conv.dilation,
                                     C.c_float(slope), L.stream()), "sa_xv_tdnn_fwd_train")
    _stale(conv)
    return z, ops.sum_partials(part, 1, n=2 * Cout)


def _stale(conv):
    """drop the cached operand images of a trained Conv1d.  torch's fused Adam updates the
    parameters in place without bumping their version counter, so the (data_ptr, _version) key of
    _packed / _packed_dgrad cannot see an optimizer step: the train path repacks every step and
    leaves the cache empty behind it, so that an eval-mode call after the step packs the new
    weights."""
    conv._img_key = conv._dimg_key = None


def _wgrad_split(M, tiles):
    """(nsplit, rows_per): ~512 workgroups, rows_per a multiple of 32."""
    nsplit = max(1, min(512 // max(1, tiles), -(-M // 256)))
    rows_per = -(-(-(-M // nsplit)) // 32) * 32
    return -(-M // rows_per), rows_per


def _tdnn_wgrad(dpre, x, s_in, t_in, conv, dW):
    lib = L.load()
    B, T, Cin = x.shape
    Cout, K, dil = conv.conv.out_channels, conv.kernel_size, conv.dilation
    nsplit, rows_per = _wgrad_split(B * T, -(-Cout // 128) * -(-Cin // 128) * K)
    part = torch.empty(nsplit, K, Cout, Cin, dtype=torch.float32, device=x.device)
    L.check(lib.sa_xv_tdnn_wgrad(L.ptr(dpre), L.ptr(x), L.ptr(s_in), L.ptr(t_in), L.ptr(part), B, T, Cin, Cout,
                                 K, dil, nsplit, rows_per, L.stream()), "sa_xv_tdnn_wgrad")
    L.check(lib.sa_xv_wgrad_reduce(L.ptr(part), nsplit, K, Cout, Cin, L.ptr(dW), L.stream()),
            "sa_xv_wgrad_reduce")
    return dW


def _tdnn_dgrad(dpre, conv):
    B, T, Cy = dpre.shape
    _stale(conv)
    return _dgrad(dpre, conv, lambda lib, img, dxe, cred, npad: L.check(
        lib.sa_xv_tdnn_dgrad(L.ptr(dpre), L.ptr(img), L.ptr(dxe), B, T, Cy, cred, conv.conv.in_channels, npad,
                             conv.kernel_size, conv.dilation, L.stream()), "sa_xv_tdnn_dgrad"))


def train_parameters(xv, cl):
    """the 30 trainable tensors in the order _XvTrainFn takes them"""
    out = []
    for conv, bn in xv.tdnn():
        out += [conv.conv.weight, conv.conv.bias, bn.norm.weight, bn.norm.bias]
    lin = xv.blocks[-1].w
    blk = cl.DNN["block_0"]
    out += [lin.weight, lin.bias, cl.norm.norm.weight, cl.norm.norm.bias, blk.linear.w.weight,
            blk.linear.w.bias, blk.norm.norm.weight, blk.norm.norm.bias, cl.out.w.weight, cl.out.w.bias]
    return out


class _XvTrainFn(torch.autograd.Function):
    """Xvector + Classifier in TRAIN mode: log-probabilities [B, classes] as a function of all 30
    parameters (BatchNorms on batch statistics, their running statistics updated).  Forward and
    backward on libsa_hip.so (sa_xvector.hip, sa_head.hip); no gradient to the features."""

    @staticmethod
    def forward(ctx, xv, cl, feats, lens, noise, *params):
        lib = L.load()
        x = feats.detach().contiguous().float()
        B, T, _ = x.shape
        zs, fs, h, s_in, t_in = [], [], x, None, None
        for conv, bn in xv.tdnn():
            z, sums = _tdnn_train(h, s_in, t_in, conv)
            f = _bn_train_stats(sums, bn.norm, B * T)
            zs.append(z)
            fs.append(f)
            h, s_in, t_in = z, f[2], f[3]
        Cc = h.shape[2]
        lens_d = _lens(lens, h.device)
        pz = _time_pool(h, lens_d, None)
        pooled = torch.empty_like(pz)
        L.check(lib.sa_xv_pool_affine(L.ptr(pz), L.ptr(s_in), L.ptr(t_in), L.ptr(noise), B, Cc, C.c_float(1e-5),
                                      L.ptr(pooled), L.stream()), "sa_xv_pool_affine")
        emb = _linear(pooled, xv.blocks[-1].w)
        blk = cl.DNN["block_0"]
        u1 = _leaky(emb)
        f1 = _bn_train_stats(_colsums(u1), cl.norm.norm, B)
        v1 = _leaky(emb, f1[2], f1[3])
        h1 = _linear(v1, blk.linear.w)
        u2 = _leaky(h1)
        f2 = _bn_train_stats(_colsums(u2), blk.norm.norm, B)
        v2 = _leaky(h1, f2[2], f2[3])
        logp = ops.log_softmax(_linear(v2, cl.out.w))
        ctx.mods = (xv, cl)
        ctx.saved = (x, zs, fs, lens_d, pz, pooled, u1, f1, v1, u2, f2, v2, logp)
        return logp

    @staticmethod
    def backward(ctx, d_logp):
        lib = L.load()
        xv, cl = ctx.mods
        x, zs, fs, lens_d, pz, pooled, u1, f1, v1, u2, f2, v2, logp = ctx.saved
        ctx.saved = None
        params = train_parameters(xv, cl)
        grads = [torch.empty_like(p) for p in params]
        B, T, _ = x.shape
        nb = len(zs)
        (gW, gb, gg1, gb1, gW1, gbl1, gg2, gb2, gWo, gbo) = grads[4 * nb:]
        blk = cl.DNN["block_0"]
        # ---- head: out Linear <- BatchNorm/LeakyReLU <- Linear <- BatchNorm/LeakyReLU <- embedding Linear
        g = ops.log_softmax_bwd(d_logp.contiguous().float(), logp)
        ops.dense_wgrad(g, v2, gWo)
        _fin_bias(_colsums(g), gbo)
        g = _linear_T(g, cl.out.w)
        gp = torch.empty_like(g)
        _fin_bias(_bn_leaky_bwd(g, u2, blk.norm.norm, f2, B, gg2, gb2, gp), gbl1)
        ops.dense_wgrad(gp, v1, gW1)
        g = _linear_T(gp, blk.linear.w)
        gp = torch.empty_like(g)
        _fin_bias(_bn_leaky_bwd(g, u1, cl.norm.norm, f1, B, gg1, gb1, gp), gb)
        ops.dense_wgrad(gp, pooled, gW)
        gpool = _linear_T(gp, xv.blocks[-1].w)
        # ---- statistics pooling of the last block's BatchNorm output
        gz = torch.empty_like(gpool)
        L.check(lib.sa_xv_pool_affine_bwd(L.ptr(gpool), L.ptr(fs[-1][2]), B, zs[-1].shape[2], L.ptr(gz), L.stream()),
                "sa_xv_pool_affine_bwd")
        dy = _time_pool_bwd(zs[-1], lens_d, gz, pz)
        # ---- TDNN blocks, last to first
        for i, (conv, bn) in reversed(list(enumerate(xv.tdnn()))):
            gw, gbias, ggam, gbet = grads[4 * i: 4 * i + 4]
            z = zs[i]
            dpre = torch.empty_like(z)
            bsum = _bn_leaky_bwd(dy.view(B * T, -1), z.view(B * T, -1), bn.norm, fs[i], B * T, ggam, gbet,
                                 dpre.view(B * T, -1))
            _fin_bias(bsum, gbias)
            xin, s_in, t_in = (x, None, None) if i == 0 else (zs[i - 1], fs[i - 1][2], fs[i - 1][3])
            _tdnn_wgrad(dpre, xin, s_in, t_in, conv, gw)
            if i > 0:
                dy = _tdnn_dgrad(dpre, conv)
            _stale(conv)
        return (None, None, None, None, None) + tuple(grads)


def train_log_probs(embedding_model, classifier, feats, lens=None):
    """log-probabilities [B, 1, classes] of Xvector -> Classifier.  With both modules in training
    mode (a mismatch raises), grad enabled and trainable parameters: the train path (_XvTrainFn; batch statistics, running
    statistics updated, pooling noise drawn per call unless ``pooling_noise`` is a tensor), which
    fills the gradients of all 30 parameters.  Otherwise the eval-mode forward."""
    if embedding_model.training != classifier.training:
        raise ValueError("embedding_model and classifier must both be in training mode or both in eval mode")
    params = train_parameters(embedding_model, classifier)
    if not (embedding_model.training and torch.is_grad_enabled() and any(p.requires_grad for p in params)):
        return classifier(embedding_model(feats, lens))
    if not feats.is_cuda:
        raise L.SaHipError("the x-vector classifier runs on the GPU only (no CPU fallback)")
    B = feats.shape[0]
    if B < 2:
        raise ValueError("Expected more than 1 value per channel when training (batch of one utterance)")
    Cc = embedding_model.tdnn()[-1][0].conv.out_channels
    noise = ops.pooling_noise(embedding_model.pooling_noise, B, Cc, feats.device)
    return _XvTrainFn.apply(embedding_model, classifier, feats, lens, noise, *params).unsqueeze(1)


class EncoderClassifier(nn.Module):
    """embedding_model + classifier with the fork's classify_batch_feats()."""

    def __init__(self, embedding_model=None, classifier=None):
        super().__init__()
        self.embedding_model = embedding_model or Xvector()
        self.classifier = classifier or Classifier()

    def forward(self, feats, wav_lens=None):
        """(log_probs [B, classes], score, index) like classify_batch_feats, but part of the
        autograd graph through `feats` (models/EndToEnd.py:81); the classifier stays frozen."""
        if not feats.is_cuda:
            raise L.SaHipError("the x-vector classifier runs on the GPU only (no CPU fallback)")
        out_prob = _XvFn.apply(self, feats, wav_lens)
        score, index = torch.max(out_prob.detach(), dim=-1)
        return out_prob, score, index

    @torch.no_grad()
    def classify_batch_feats(self, feats, wav_lens=None):
        out_prob = self.classifier(self.embedding_model(feats, wav_lens)).squeeze(1)
        score, index = torch.max(out_prob, dim=-1)
        return out_prob, score, index
