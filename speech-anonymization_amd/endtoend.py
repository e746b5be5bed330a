"""ConvReconstruction: drop-in for ``models.EndToEnd.ConvReconstruction`` of the reference
(models/EndToEnd.py:36-87, BASELINE config 4 / SURVEY 8f-1) with forward + backward on libsa_hip.so.

  feats [B, T, 80] -> reshape [B, 1, T*80] -> encoder (:40-54):
      Conv1d(1->32, k15, p7) -> InstanceNorm(32) -> x*sigmoid(x) -> Conv1d(32->64, k5, s2, p2) -> IN(64) -> act
      -> Conv1d(64->64, k5, p2) -> IN(64) -> act -> ConvTranspose1d(64->32, k5, s2, p2, op1) -> IN(32) -> act
      -> Conv1d(32->1, k15, p7)                                    -> recon [B, T, 80]
  sex_classifier (:57-61,81): the PRETRAINED, frozen x-vector EncoderClassifier applied to the
      reconstruction -> (log_probs, score, index); only the gradient with respect to the
      reconstruction flows back (xvector.EncoderClassifier.forward).

Same parameter names / shapes as the reference module (``encoder.0.weight`` ... ``encoder.12.bias``;
the torch.nn layers are parameter containers only).  The conv stack is a subset of the
ConvAutoencoder's kernels (sa_conv1toC / sa_conv_gemm 32->64 s2, 64->64, ConvT 64->32 /
sa_convCto1, statistics in the producers' epilogues, normalisation + activation in the consumers'
prologues); the backward uses the two-pass normalisation backward (statistics in the data-gradient
epilogue, sa_ew_apply) -- this "next" row is built for parity first.

The reference constructs the classifier from absolute paths on its authors' machine
(``EncoderClassifier.from_hparams(source="/home/ubuntu/...")``, :57-61); here it is passed in
(``ConvReconstruction(sex_classifier=...)``) or built with random weights.
"""
import functools
import os

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._lib import SaHipError
from .convae import GLU, _in_ep
from .xvector import EncoderClassifier


class ConvReconstruction(nn.Module):
    def __init__(self, sex_classifier=None, precision="bf16x3"):
        super().__init__()
        if precision not in ("bf16x3", "f32"):
            raise SaHipError("ConvReconstruction runs in precision bf16x3 or f32")
        self.precision = precision
        self.act_dtype, self.kcode = ops.PRECISIONS[precision]
        # encoder.12's data gradient and weight gradient in one launch (ConvAutoencoder.fused_bwd1c)
        self.fused_bwd1c = os.environ.get("SA_FUSED_BWD1C", "1") == "1"
        self.encoder = nn.Sequential(
            nn.Conv1d(1, 32, 15, 1, 7), nn.InstanceNorm1d(32, affine=True), GLU(),
            nn.Conv1d(32, 64, 5, 2, 2), nn.InstanceNorm1d(64, affine=True), GLU(),
            nn.Conv1d(64, 64, 5, 1, 2), nn.InstanceNorm1d(64, affine=True), GLU(),
            nn.ConvTranspose1d(64, 32, 5, 2, 2, output_padding=1), nn.InstanceNorm1d(32, affine=True), GLU(),
            nn.Conv1d(32, 1, 15, 1, 7),
        )
        self.lay = ops.conv_layers(self, ("encoder",))        # the conv_gemm layers' launch geometry, stated once
        self.sex_classifier = sex_classifier if sex_classifier is not None else EncoderClassifier()
        for p in self.sex_classifier.parameters():          # pretrained and frozen in the reference
            p.requires_grad = False
        self.sex_classifier.eval()

    def train(self, mode=True):
        super().train(mode)
        self.sex_classifier.eval()                          # BatchNorm running statistics, always
        return self

    @torch.no_grad()
    def reconstruct(self, feats):
        """recon [B, T, 80] for inference: the conv stack's launches with forward's arguments, hence the bits
        of ``model(feats)[0]`` in train and eval mode alike (InstanceNorm only).  The frozen x-vector does not
        run and nothing is kept for a backward.  Refuses what forward refuses."""
        if not torch.is_tensor(feats) or feats.dim() != 3:
            raise SaHipError("ConvReconstruction expects feats [B, T, 80]")
        x0, B, T, Ltot = _input_rows(feats)
        P = {k: p for k, p in self.named_parameters() if k.startswith("encoder.")}
        return _recon_launches(self, P, x0, B, Ltot)[2].view(B, T, 80)

    def forward(self, feats):
        names, params = zip(*((k, p) for k, p in self.named_parameters() if k.startswith("encoder.")))
        recon = _ConvRecFn.apply(self, names, feats, *params)
        logp, score, index = self.sex_classifier(recon)
        return recon, logp


def _input_rows(feats):
    """feats [B, T, 80] -> (x0 [B, T*80] fp32, B, T, T*80); the refusals of forward and reconstruct"""
    B, T, Fd = feats.shape
    Ltot = T * Fd
    if Fd != 80 or Ltot % 2:
        raise SaHipError("ConvReconstruction expects feats [B, T, 80]")
    if not feats.is_cuda:
        raise SaHipError("ConvReconstruction runs on the GPU only (no CPU fallback)")
    return feats.detach().reshape(B, Ltot).contiguous().float(), B, T, Ltot


def _cg(model, P, ly, x, dgrad=False, **kw):
    """the layer's forward launch, or its data-gradient launch on d y = x; the weights are packed per call"""
    w = ops.pack_weights(P[ly.key].detach(), ly.kinds[dgrad], model.act_dtype, model.kcode)
    args = (None,) + ly.dgrad(ly.lin(x.shape[1])) if dgrad else (P[ly.bias],) + ly.fwd(x.shape[1])
    return ops.conv_gemm(x, w, *args, code=model.kcode, **kw)


def _recon_launches(model, P, x0, B, Ltot):
    """the conv stack's launches -> ([y0..y3], [n0..n3], recon [B, Ltot]); what forward and reconstruct run"""
    L2, lay = Ltot // 2, model.lay

    def inorm(stats, n, prefix, C):
        return ops.fin_in_fwd(ops.sum_partials(stats, B), B, C, n, P[prefix + ".weight"], P[prefix + ".bias"])

    y0, st = ops.conv1toC(x0, P["encoder.0.weight"], P["encoder.0.bias"], model.act_dtype, want_stats=True)
    n0 = inorm(st, Ltot, "encoder.1", 32)
    y1, st = _cg(model, P, lay["encoder.3"], y0, s1=n0[2], t1=n0[3], swish=True, want_stats=True)
    n1 = inorm(st, L2, "encoder.4", 64)
    y2, st = _cg(model, P, lay["encoder.6"], y1, s1=n1[2], t1=n1[3], swish=True, want_stats=True)
    n2 = inorm(st, L2, "encoder.7", 64)
    y3, st = _cg(model, P, lay["encoder.9"], y2, s1=n2[2], t1=n2[3], swish=True, want_stats=True)
    n3 = inorm(st, Ltot, "encoder.10", 32)
    recon = ops.convCto1(y3, P["encoder.12.weight"], P["encoder.12.bias"], n3[2], n3[3], True)
    return [y0, y1, y2, y3], [n0, n1, n2, n3], recon


class _ConvRecFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, names, feats, *params):
        ctx.set_materialize_grads(False)
        x0, B, T, Ltot = _input_rows(feats)
        y, n, recon = _recon_launches(model, dict(zip(names, params)), x0, B, Ltot)
        ctx.S = dict(x0=x0, y=y, n=n, dims=(B, T, Ltot, Ltot // 2))
        ctx.model, ctx.names, ctx.params = model, names, params
        ctx.need_input_grad = feats.requires_grad
        return recon.view(B, T, 80)

    @staticmethod
    def backward(ctx, d_recon):
        S, model, names = ctx.S, ctx.model, ctx.names
        if S is None:
            raise SaHipError("ConvReconstruction backward called twice (saved tensors were released)")
        P = dict(zip(names, ctx.params))
        dt, lay = model.act_dtype, model.lay
        B, T, Ltot, L2 = S["dims"]
        y0, y1, y2, y3 = S["y"]
        n0, n1, n2, n3 = S["n"]
        dev = y0.device
        G = {k: None for k in names}
        need = {k: p.requires_grad for k, p in P.items()}
        if d_recon is None:
            ctx.S = None
            return (None, None, None) + tuple(None for _ in names)
        wg = functools.partial(ops.wgrad, code=ops.WGRAD_CODE[model.precision])

        def newg(key):
            return torch.empty_like(P[key])

        def layer_bwd(ly, x, nrm, dy):
            """the layer's weight gradient (x, nrm: its stored input and that input's norm), then d z of its input"""
            if need[ly.key]:
                *geo, strides = ly.wgrad(x.shape[1])
                G[ly.key] = wg(x, dy, *geo, newg(ly.key), strides, s1=nrm[2], t1=nrm[3], swish=True)
            return _cg(model, P, ly, dy, dgrad=True, want_stats=True, ep=_in_ep(x, nrm))

        def norm_bwd(g, st, y, nrm, C, Ln, prefix, bias_key):
            """g = d z (already multiplied by the activation derivative), st = partial (sum dz,
            sum dz*xhat): InstanceNorm backward coefficients, then d y = c1*dz + c2*y + c3 in place;
            also the gradients of the norm's affine parameters and of the conv bias in front."""
            sums = ops.sum_partials(st, B)
            dg, db = newg(prefix + ".weight"), newg(prefix + ".bias")
            c1, c2, c3 = ops.fin_norm_bwd(sums, sums, B * C, C, Ln, P[prefix + ".weight"], nrm[0], nrm[1],
                                          dgamma=dg, dbeta=db)
            G[prefix + ".weight"], G[prefix + ".bias"] = dg, db
            st2 = ops.ew("apply", g, y, C, out=g, c1=c1, c2=c2, c3=c3)
            if need[bias_key]:
                G[bias_key] = ops.fin_bias(ops.sum_partials(st2, B), B, C, newg(bias_key))
            return g

        g_rec = d_recon.reshape(B, Ltot).contiguous().float()
        if need["encoder.12.bias"]:
            G["encoder.12.bias"] = ops.sum_partials(g_rec.view(4 * B, Ltot // 4), 1, n=Ltot // 4).sum().float().reshape(1)
        if need["encoder.12.weight"] and model.fused_bwd1c:
            g, st, G["encoder.12.weight"] = ops.bwd1C(g_rec, y3, P["encoder.12.weight"], newg("encoder.12.weight"),
                                                      n3[2], n3[3], n3[0], n3[1])                 # d z3
        else:
            if need["encoder.12.weight"]:
                G["encoder.12.weight"] = ops.wgrad1C(g_rec, y3, newg("encoder.12.weight"), flip=True,
                                                     s1=n3[2], t1=n3[3], swish=True)
            g, st = ops.conv1toC(g_rec, P["encoder.12.weight"], None, dt, flip=True, want_stats=True,
                                 ep=dict(x=y3, s1=n3[2], t1=n3[3], mean=n3[0], rstd=n3[1]))      # d z3
        g = norm_bwd(g, st, y3, n3, 32, Ltot, "encoder.10", "encoder.9.bias")                    # d y3
        g, st = layer_bwd(lay["encoder.9"], y2, n2, g)                                           # d z2
        g = norm_bwd(g, st, y2, n2, 64, L2, "encoder.7", "encoder.6.bias")                       # d y2
        g, st = layer_bwd(lay["encoder.6"], y1, n1, g)                                           # d z1
        g = norm_bwd(g, st, y1, n1, 64, L2, "encoder.4", "encoder.3.bias")                       # d y1
        g, st = layer_bwd(lay["encoder.3"], y0, n0, g)                                           # d z0
        g = norm_bwd(g, st, y0, n0, 32, Ltot, "encoder.1", "encoder.0.bias")                     # d y0
        if need["encoder.0.weight"]:
            G["encoder.0.weight"] = ops.wgrad1C(S["x0"], g, newg("encoder.0.weight"))
        d_feats = None
        if ctx.need_input_grad:
            d_feats = ops.convCto1(g, P["encoder.0.weight"], None, flip=True).view(B, T, 80)
        ctx.S = None
        return (None, None, d_feats) + tuple(G[k] if need[k] else None for k in names)
