"""ConvAutoencoder: drop-in for ``models.ConvAutoEncoder.ConvAutoencoder`` of the reference
(models/ConvAutoEncoder.py:136-200) with the whole forward + backward on libsa_hip.so.

Same constructor (no arguments needed), same ``forward(feats[B,T,80]) -> (recon[B,T,80],
log_probs[B,2])``, same parameter / buffer names and shapes (``encoder.0.weight`` ...
``sex_classifier.classify.6.bias``; the torch.nn layers below are used ONLY as parameter
containers so that ``state_dict()``, ``named_parameters()`` with the reference's
``"sex_classifier" in name`` freeze logic, and default initialisation are the reference's).
Their ``forward`` is never called: one ``torch.autograd.Function`` runs the fused pipeline
  - activations channels-last [B, L, C] in ``dtype`` (bf16 default, fp32 available),
  - InstanceNorm / BatchNorm statistics from the producing conv's epilogue, normalisation +
    x*sigmoid(x) applied in the consumer's prologue (the normalised tensors are never stored),
  - GradReverse folded into the first classifier BatchNorm's backward coefficients,
  - the reshape-not-transpose before StatisticsPooling (models/ConvAutoEncoder.py:61).
"""
import functools
import os

import torch
import torch.nn as nn

from . import distributed as sdist
from . import ops
from . import _lib as L
from ._lib import SaHipError


class _ParamOnly(nn.Module):
    """activation placeholders keep the Sequential indices of the reference."""

    def forward(self, x):                                        # pragma: no cover
        raise SaHipError("parameter container only; use ConvAutoencoder.forward")


class GLU(_ParamOnly):
    pass


class StatisticsPooling(_ParamOnly):
    pass


class TDNNSexClassifier(nn.Module):
    def __init__(self, num_classes=2):
        super().__init__()
        self.tdnn = nn.Sequential(
            nn.Conv1d(128, 128, kernel_size=5, dilation=1), nn.ReLU(), nn.BatchNorm1d(128),
            nn.Conv1d(128, 128, kernel_size=3, dilation=2), nn.ReLU(), nn.BatchNorm1d(128),
            nn.Conv1d(128, 128, kernel_size=3, dilation=3), nn.ReLU(), nn.BatchNorm1d(128),
        )
        self.norm = nn.BatchNorm1d(128)
        self.stats_pooling = StatisticsPooling()
        self.classify = nn.Sequential(
            nn.Linear(256, 128), nn.ReLU(), nn.BatchNorm1d(128),
            nn.Linear(128, 64), nn.ReLU(), nn.BatchNorm1d(64),
            nn.Linear(64, num_classes),
        )

    def forward(self, x):                                        # pragma: no cover
        raise SaHipError("parameter container only; use ConvAutoencoder.forward")


class ConvAutoencoder(nn.Module):
    def __init__(self, precision="bf16x3", pooling_noise=True, sync_bn=True, dtype=None,
                 cache_wgrad_operand=True):
        """precision: "bf16x3" (default: fp32 storage, split-bf16 operands on the bf16 MFMA --
        meets the 1e-4 parity bar), "bf16" (bf16 storage + single bf16 MFMA: fastest, ~2e-4 on
        recon), "f32" (exact fp32 MFMA).  dtype=torch.float32 / torch.bfloat16 selects "f32" /
        "bf16" (kept for callers that think in torch dtypes).  cache_wgrad_operand=False trades
        the bf16 operand cache (memory) for recomputation in the weight-gradient kernels."""
        super().__init__()
        if dtype is not None:
            precision = {torch.float32: "f32", torch.bfloat16: "bf16"}[dtype]
        if precision not in ops.PRECISIONS:
            raise SaHipError(f"unknown precision {precision!r}")
        self.precision = precision
        self.encoder = nn.Sequential(
            nn.Conv1d(1, 32, 15, 1, 7), GLU(),
            nn.Conv1d(32, 64, 5, 2, 2), nn.InstanceNorm1d(64, affine=True), GLU(),
            nn.Conv1d(64, 64, 5, 1, 2), nn.InstanceNorm1d(64, affine=True), GLU(),
            nn.Conv1d(64, 128, 5, 2, 2), nn.InstanceNorm1d(128, affine=True), GLU(),
            nn.Conv1d(128, 128, 5, 1, 2), nn.InstanceNorm1d(128, affine=True), GLU(),
        )
        self.decoder = nn.Sequential(
            nn.Conv1d(128, 128, 5, 1, 2),
            nn.ConvTranspose1d(128, 64, 5, 2, 2, output_padding=1),
            nn.InstanceNorm1d(64, affine=True), GLU(),
            nn.Conv1d(64, 64, 5, 1, 2),
            nn.ConvTranspose1d(64, 32, 5, 2, 2, output_padding=1),
            nn.InstanceNorm1d(32, affine=True), GLU(),
            nn.Conv1d(32, 1, 15, 1, 7),
        )
        self.sex_classifier = TDNNSexClassifier(2)
        # every conv_gemm layer's launch geometry, derived from the containers above
        self.lay = ops.conv_layers(self, ("encoder", "sex_classifier.tdnn", "decoder"))
        # every (weight, use) pair the fused forward / backward multiplies with: the forward images, Conv1d before
        # ConvTranspose1d, then the data-gradient images in the same order
        self.pack_plan = [(ly.key, ly.kinds[i]) for i in (0, 1)
                          for ly in sorted(self.lay.values(), key=lambda ly: ly.transposed)]
        self.act_dtype, self.kcode = ops.PRECISIONS[precision]
        # kernel precision of the data-gradient convolutions (tools/precision_probe.py overrides it)
        self.dgrad_kcode = ops.DGRAD_CODE[precision]
        # forward convs also store their transformed input in bf16 for the weight gradient
        # (bf16x3 / bf16x1f models; +1/2 of the saved activations in memory, identical results).
        # With the cache and a bf16x3 / bf16 data gradient the norm-backward apply passes run in the
        # prologue of the data-gradient convolutions; otherwise as separate sa_ew_apply launches.
        self.cache_wgrad_operand = cache_wgrad_operand
        # speechbrain's StatisticsPooling adds eps*U[1,9] to the pooled mean on every call
        # (train and eval); True reproduces that, a tensor [B,128] in [0,1] fixes the draw
        # (tests), False/None gives the deterministic form the oracle uses.
        self.pooling_noise = pooling_noise
        self.sync_bn = sync_bn
        # The kernels of a step are issued on one stream, reductions and finalisers as separate launches,
        # the bias gradients and split-K reducers of a backward stage batched at its end: DESIGN.md has
        # the measurements behind each.  The two switches below both have a live off path.
        # the FC head as one forward and one backward launch (sa_head_fused.hip) where its BatchNorm
        # statistics are local and B fits one workgroup; SA_FUSED_HEAD=0: the separate launches
        self.fused_head = os.environ.get("SA_FUSED_HEAD", "1") == "1"
        # decoder.8's data gradient and weight gradient from one read of y8 (sa_bwd1C; same bits);
        # SA_FUSED_BWD1C=0: the two launches (conv1toC + wgrad1C)
        self.fused_bwd1c = os.environ.get("SA_FUSED_BWD1C", "1") == "1"
        # the pooling finaliser in the tail of the gather launch, the noise draw normalised there instead of on
        # four ATen kernels (sa_pool_gather_fin; same bits); SA_FUSED_POOL_FIN=0: gather + finaliser launches
        self.fused_pool_fin = os.environ.get("SA_FUSED_POOL_FIN", "1") == "1"
        # the fused head's backward over 16 workgroups, each with a slice of d W1 / d W2 / d pooled
        # (sa_head_bwd_wide; same bits); SA_WIDE_HEAD_BWD=0: the one-workgroup launch (sa_head_bwd)
        self.wide_head_bwd = os.environ.get("SA_WIDE_HEAD_BWD", "1") == "1"
        # data-parallel FC head: None = every BatchNorm1d of the head exchanges its sums (any batch
        # split); "equal" = every rank holds a batch as large as this one (what data.shard_indices
        # deals); [b0, b1, ...] = the ranks' batch sizes.  With the sizes known the pooled rows are
        # exchanged ONCE and the head runs on the global batch on every rank (_head_plan).
        self.dp_batch_sizes = None

    def forward(self, feats):
        # walking the module tree costs ~0.15 ms a call: the (names, parameters) lists are cached
        # and revalidated against the owners' registries (56 identity checks, ~5 us), so replacing
        # ANY parameter object (load into a sub-module, .to(), pruning, ...) is noticed
        names, params = self._named_params()
        return _ConvAEFn.apply(self, names, feats, *params)

    def _named_params(self):
        c = self.__dict__.get("_np_cache")
        if c is None or any(o[n] is not p for o, n, p in c[2]):
            names, params, owners = [], [], []
            for mname, mod in self.named_modules():
                for pname, p in mod._parameters.items():
                    if p is not None:
                        names.append(f"{mname}.{pname}" if mname else pname)
                        params.append(p)
                        owners.append((mod._parameters, pname, p))
            c = self.__dict__["_np_cache"] = (tuple(names), tuple(params), owners)
        return c[0], c[1]

    @torch.no_grad()
    def reconstruct(self, feats):
        """recon [B, T, 80] for inference: the launches of the eval-mode forward's reconstruction path
        (conv1toC, the eight convolutions, convCto1, the InstanceNorm finalisers) with the same arguments,
        hence the bits of ``model.eval(); model(feats)[0]`` -- in train mode too, since this path holds only
        InstanceNorm.  The classifier branch does not run: no running statistic or step counter moves,
        nothing is kept for a backward.  Refuses what forward refuses."""
        if not torch.is_tensor(feats) or feats.dim() != 3:
            raise SaHipError("ConvAutoencoder expects feats [B, T, 80]")
        x0, B, T, Ltot = _input_rows(feats)
        P = dict(zip(*self._named_params()))
        cg, inorm = _launchers(self, P, _packed(self, P), B)
        y, _, _ = _encoder_launches(self, P, cg, inorm, x0, Ltot, False)
        return _decoder_launches(self, P, cg, inorm, y[5], Ltot)[-1].view(B, T, 80)

    def _side_stream(self, device):
        if getattr(self, "_side", None) is None and device.type == "cuda":
            self._side = torch.cuda.Stream(device=device)
        return getattr(self, "_side", None)

    # ---- SyncBatchNorm support: statistics sums are all-reduced across data-parallel ranks
    # (what speechbrain's Brain applies under DDP); identity on one process.
    def _bn_syncs(self):
        return self.sync_bn and sdist.dp_active()

    def _bn_allreduce(self, sums):
        if self._bn_syncs():
            sdist.all_reduce_now(sums)
            return sdist.world_size()
        return 1

    def _bn_global_counts(self, counts, device):
        """SyncBatchNorm element counts.  Ranks hold ragged batches (data.batches pads each rank's
        batch to its own longest utterance, the last batch may be short), so the per-layer counts
        are all-reduced beside the sums -- torch.nn.SyncBatchNorm, which speechbrain applies for
        the reference under DDP, exchanges counts the same way.  ONE collective per step for the
        six BatchNorms; the result stays on the device (the finalisers read it there:
        sa_fin_bn_fwd / sa_fin_norm_bwd / sa_bn2d_bwd `count_dev`).  None on a single process."""
        if not self._bn_syncs():
            return None
        key = (tuple(counts), str(device))
        cache = self.__dict__.setdefault("_count_cache", {})
        local = cache.get(key)
        if local is None:
            if len(cache) > 64:
                cache.clear()
            local = cache[key] = torch.tensor(counts, dtype=torch.float64).to(device)
        g = local.clone()
        sdist.all_reduce_now(g)
        return g

    def _bn_rows(self):
        """per-utterance partial rows may go straight to the finalisers when nothing is all-reduced"""
        return not self._bn_syncs()

    def _bn_global(self, local_sums):
        """(global sums, world): the all-reduced copy of the local sums, or the local sums
        themselves on one process (no copy)."""
        if not self._bn_syncs():
            return local_sums, 1
        g = local_sums.clone()
        return g, self._bn_allreduce(g)

    def _head_plan(self, B):
        """(row offset of this rank, global batch, world) when the FC head runs on the gathered
        global batch, else None.  The two BatchNorm1d exchanges of the forward and the two of the
        backward become one exchange of the pooled rows [B_global, 256] and one of d log p
        [B_global, 2]; the statistics are then local sums over the global rows."""
        if not self._bn_syncs() or self.dp_batch_sizes is None:
            return None
        W, r = sdist.world_size(), sdist.rank()
        sizes = [B] * W if isinstance(self.dp_batch_sizes, str) else [int(b) for b in self.dp_batch_sizes]
        if self.dp_batch_sizes != "equal" and isinstance(self.dp_batch_sizes, str):
            raise SaHipError(f"dp_batch_sizes: 'equal', a list of per-rank batch sizes or None, not {self.dp_batch_sizes!r}")
        if len(sizes) != W or sizes[r] != B:
            raise SaHipError(f"dp_batch_sizes {sizes} does not describe rank {r} of {W} holding {B} utterances")
        return sum(sizes[:r]), sum(sizes), W

    @staticmethod
    def _gather_rows(x, plan):
        """[B_global, C] with every rank's rows in rank order: this rank's rows into a zeroed
        buffer, one sum all-reduce (adds exact zeros, so the rows arrive bit-identical)."""
        off, Bg, _ = plan
        g = torch.zeros(Bg, x.shape[1], device=x.device, dtype=x.dtype)
        g[off:off + x.shape[0]].copy_(x)
        sdist.all_reduce_now(g)
        return g


class _W:
    """packed weight image + the kernel precision code it was packed for"""
    __slots__ = ("img", "code")

    def __init__(self, img, code):
        self.img, self.code = img, code


def _kcode(model, kind):
    return model.dgrad_kcode if kind.endswith("dgrad") else model.kcode


def _packed(model, P):
    """All operand images of the current weights, refreshed by ONE launch.  The image buffers
    are persistent (keyed by the parameters' storage): a backward uses the images its forward
    packed, which is what autograd's saved-tensor semantics ask for as long as the weights are
    not modified between the two."""
    items = [((k, kind), P[k], kind, _kcode(model, kind)) for k, kind in model.pack_plan]
    key = tuple(w.data_ptr() for _, w, _, _ in items) + tuple(c for _, _, _, c in items)
    pk = getattr(model, "_pack_cache", None)
    if pk is None or pk[0] != key:
        pk = (key, ops.PackedWeights(items, model.act_dtype))
        model._pack_cache = pk
    pk[1].refresh()
    return {tag: _W(img, code) for tag, (img, code) in pk[1].images.items()}


def _conv(x, w, *args, **kw):
    return ops.conv_gemm(x, w.img, *args, code=w.code, **kw)


class _PendingApply:
    """d z of a normalised layer together with the coefficients of d y = c1*dz + c2*y + c3 that the
    next data-gradient convolution applies in its prologue (instead of a sa_ew_apply pass)."""
    __slots__ = ("g", "y", "c", "per_c", "relu", "bias_key", "wgrads")

    def __init__(self, g, y, c, per_c, relu, bias_key):
        self.g, self.y, self.c, self.per_c, self.relu, self.bias_key = g, y, c, per_c, relu, bias_key
        self.wgrads = []


def _noise(model, B, device):
    return ops.pooling_noise(model.pooling_noise, B, 128, device)


def _input_rows(feats):
    """feats [B, T, 80] -> (x0 [B, T*80] fp32, B, T, T*80); the refusals of forward and reconstruct"""
    B, T, Fd = feats.shape
    Ltot = T * Fd
    if Fd != 80 or Ltot % 4:
        raise SaHipError("ConvAutoencoder expects feats [B, T, 80] with T*80 divisible by 4")
    if not feats.is_cuda:
        raise SaHipError("ConvAutoencoder runs on the GPU only (no CPU fallback)")
    return feats.detach().reshape(B, Ltot).contiguous().float(), B, T, Ltot


def _in_ep(y, nrm, g2=None):
    """fused-epilogue description of an [InstanceNorm -> swish] backward (stats pass)."""
    mean, rstd, scale, shift = nrm
    d = dict(mode=1, x=y, g2=g2, s1=scale, t1=shift, mean=mean, rstd=rstd)
    if isinstance(g2, _PendingApply):                     # apply of the `norm` BatchNorm rides along
        d.update(g2=g2.g, g2k=g2.c)
    return d


def _launchers(model, P, W, B, A=None):
    """(cg, inorm): a layer's forward launch and an InstanceNorm finaliser as forward and reconstruct issue them.
    W: the packed images (_packed).  A: dict that receives the bf16 operand cache of the weight gradients (None:
    no cache)."""
    def cg(ly, x, **kw):
        if A is not None and P[ly.key].requires_grad:
            A[ly.key] = kw["a_out"] = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        return _conv(x, W[ly.key, ly.kinds[0]], P[ly.bias], *ly.fwd(x.shape[1]), **kw)

    def inorm(stats, n, prefix, C):
        sums = ops.sum_partials(stats, B)
        return ops.fin_in_fwd(sums, B, C, n, P[prefix + ".weight"], P[prefix + ".bias"])
    return cg, inorm


def _encoder_launches(model, P, cg, inorm, x0, Ltot, want_pro_stats):
    """encoder + decoder.0 -> ([y0..y5], [n1..n4], a4_stats or None).  decoder.0 belongs here: it stages the
    transformed encoder output, and in train mode leaves the statistics the classifier's input BatchNorm
    needs as a by-product of its prologue (want_pro_stats)."""
    L2, L4, lay = Ltot // 2, Ltot // 4, model.lay
    y0 = ops.conv1toC(x0, P["encoder.0.weight"], P["encoder.0.bias"], model.act_dtype)
    y1, st = cg(lay["encoder.2"], y0, swish=True, want_stats=True)
    n1 = inorm(st, L2, "encoder.3", 64)
    y2, st = cg(lay["encoder.5"], y1, s1=n1[2], t1=n1[3], swish=True, want_stats=True)
    n2 = inorm(st, L2, "encoder.6", 64)
    y3, st = cg(lay["encoder.8"], y2, s1=n2[2], t1=n2[3], swish=True, want_stats=True)
    n3 = inorm(st, L4, "encoder.9", 128)
    y4, st = cg(lay["encoder.11"], y3, s1=n3[2], t1=n3[3], swish=True, want_stats=True)
    n4 = inorm(st, L4, "encoder.12", 128)
    y5 = cg(lay["decoder.0"], y4, s1=n4[2], t1=n4[3], swish=True, want_pro_stats=want_pro_stats)
    a4_stats = None
    if want_pro_stats:
        y5, a4_stats = y5
    return [y0, y1, y2, y3, y4, y5], [n1, n2, n3, n4], a4_stats


def _decoder_launches(model, P, cg, inorm, y5, Ltot):
    """decoder.1 ... decoder.8 -> (y6, n6, y7, y8, n8, recon [B, Ltot])"""
    L2, lay = Ltot // 2, model.lay
    y6, st = cg(lay["decoder.1"], y5, want_stats=True)
    n6 = inorm(st, L2, "decoder.2", 64)
    y7 = cg(lay["decoder.4"], y6, s1=n6[2], t1=n6[3], swish=True)
    y8, st = cg(lay["decoder.5"], y7, want_stats=True)
    n8 = inorm(st, Ltot, "decoder.6", 32)
    recon = ops.convCto1(y8, P["decoder.8.weight"], P["decoder.8.bias"], n8[2], n8[3], True)
    return y6, n6, y7, y8, n8, recon


class _ConvAEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, names, feats, *params):
        # an output the loss does not use arrives as None in backward (not as a zero tensor): the
        # parameters that only feed it then get no gradient at all, like in the reference's graph
        ctx.set_materialize_grads(False)
        P = dict(zip(names, params))
        train = model.training
        x0, B, T, Ltot = _input_rows(feats)
        L2, L4 = Ltot // 2, Ltot // 4
        S = {}                                                  # saved for backward
        W, lay = _packed(model, P), model.lay
        # activation cache: each conv also writes its transformed input rows in bf16, the operand
        # its weight gradient multiplies with (saves the recomputation and half of the bytes there)
        A = {}
        cache_a = (train and model.cache_wgrad_operand and any(ctx.needs_input_grad)
                   and ops.WGRAD_CODE[model.precision] in (L.BF16X1F, L.BF16) and model.kcode != L.FP8)

        cg, inorm = _launchers(model, P, W, B, A if cache_a else None)

        def bn_stats(stats, count, mod, prefix, C, ci):
            """train-mode BatchNorm from the per-tile partial statistics of the producing launch"""
            sums = ops.sum_partials(stats, 1, rows=model._bn_rows()) if train else None
            return bnorm(sums, count, mod, prefix, C, ci)

        def bnorm(sums, count, mod, prefix, C, ci, local=False):
            """sums [C,2] local; returns (mean, rstd, scale, shift) per channel.  ci: index of
            this BatchNorm in the all-reduced count vector gc (SyncBatchNorm).  local: the sums
            already cover the global batch (gathered head rows), nothing to exchange."""
            if not train:
                return ops.fin_bn_eval(C, P[prefix + ".weight"], P[prefix + ".bias"],
                                       mod.running_mean, mod.running_var)
            if not local:
                model._bn_allreduce(sums)
            out = ops.fin_bn_fwd(sums, C, count, P[prefix + ".weight"], P[prefix + ".bias"],
                                 mod.running_mean, mod.running_var, count_dev=None if local else cdev(ci))
            tracked.append(mod.num_batches_tracked)
            return out

        tracked = []                                            # BatchNorm step counters, bumped together
        enc, dec, cls = model.encoder, model.decoder, model.sex_classifier
        La, Lb, Lc = L4 - 4, L4 - 8, L4 - 14
        # global element counts of the six BatchNorms (norm, tdnn.2/5/8, classify.2/5) under
        # SyncBatchNorm: one tiny all-reduce, device-resident; None on one process
        gc = model._bn_global_counts([B * L4, B * La, B * Lb, B * Lc, B, B], feats.device) if train else None
        cdev = lambda i: None if gc is None else gc[i:i + 1]
        # ---------------- encoder (and decoder.0: it stages the same transformed encoder output the
        # classifier's input BatchNorm needs statistics of) ----------------
        (y0, y1, y2, y3, y4, y5), (n1, n2, n3, n4), a4_stats = _encoder_launches(model, P, cg, inorm, x0, Ltot, train)
        # ---------------- sex classifier (GradReverse = identity forward) ----------------
        bn_n = bn_stats(a4_stats if train else None, B * L4, cls.norm, "sex_classifier.norm", 128, 0)
        r0, st = cg(lay["sex_classifier.tdnn.0"], y4, s1=n4[2], t1=n4[3], swish=True, s2=bn_n[2], t2=bn_n[3],
                    relu=True, want_stats=True)
        bn0 = bn_stats(st, B * La, cls.tdnn[2], "sex_classifier.tdnn.2", 128, 1)
        r1, st = cg(lay["sex_classifier.tdnn.3"], r0, s2=bn0[2], t2=bn0[3], relu=True, want_stats=True)
        bn1 = bn_stats(st, B * Lb, cls.tdnn[5], "sex_classifier.tdnn.5", 128, 2)
        r2, st = cg(lay["sex_classifier.tdnn.6"], r1, s2=bn1[2], t2=bn1[3], relu=True, want_stats=True)
        bn2 = bn_stats(st, B * Lc, cls.tdnn[8], "sex_classifier.tdnn.8", 128, 3)
        if model.fused_pool_fin:
            nz, raw = ops.pooling_noise_raw(model.pooling_noise, B, 128, feats.device)
            pooled, pmean, psd = ops.pool_fwd(r2, bn2[2], bn2[3], noise=nz, fused=True, raw=raw)
        else:
            pooled, pmean, psd = ops.pool_fwd(r2, bn2[2], bn2[3], noise=_noise(model, B, feats.device))
        def head_fwd(X, n, local=False):
            H1 = ops.dense(X, P["sex_classifier.classify.0.weight"], P["sex_classifier.classify.0.bias"],
                           128, 256, relu=True)
            f1 = bnorm(ops.colsums(H1) if train else None, n, cls.classify[2], "sex_classifier.classify.2", 128, 4, local)
            H2 = ops.dense(H1, P["sex_classifier.classify.3.weight"], P["sex_classifier.classify.3.bias"],
                           64, 128, ps=f1[2], pt=f1[3], relu=True)
            f2 = bnorm(ops.colsums(H2) if train else None, n, cls.classify[5], "sex_classifier.classify.5", 64, 5, local)
            logits = ops.dense(H2, P["sex_classifier.classify.6.weight"], P["sex_classifier.classify.6.bias"],
                               2, 64, ps=f2[2], pt=f2[3])
            return H1, f1, H2, f2, ops.log_softmax(logits)

        # data-parallel with known per-rank batch sizes: the pooled rows of all ranks, one exchange
        plan = model._head_plan(B) if train else None
        head_in, Bh = (model._gather_rows(pooled, plan), plan[1]) if plan else (pooled, B)
        # one launch for the whole head where the batch statistics are local (train mode, no
        # SyncBatchNorm exchange between the layers) and the batch fits one workgroup
        fused_head = (train and model.fused_head and (plan is not None or not model._bn_syncs())
                      and Bh <= ops.head_max_rows())
        clsP = {k[len("sex_classifier.classify."):]: v for k, v in P.items() if k.startswith("sex_classifier.classify.")}
        if fused_head:
            H1, f1, H2, f2, logp = ops.head_fwd(head_in, clsP, cls.classify[2], cls.classify[5])
            tracked += [cls.classify[2].num_batches_tracked, cls.classify[5].num_batches_tracked]
        else:
            H1, f1, H2, f2, logp = head_fwd(head_in, Bh, plan is not None)
        logp_all = logp
        if plan:                               # this rank's rows of the global log-probabilities
            logp = logp_all[plan[0]:plan[0] + B]
        # the BatchNorm step counters: all of them are known here, and issued before the decoder the bump does
        # not sit between the forward's last kernel and the losses
        if tracked:
            torch._foreach_add_(tracked, 1)
        # ---------------- decoder ----------------
        y6, n6, y7, y8, n8, recon = _decoder_launches(model, P, cg, inorm, y5, Ltot)

        S.update(x0=x0, y=[y0, y1, y2, y3, y4, y5, y6, y7, y8], r=[r0, r1, r2],
                 n=[None, n1, n2, n3, n4, None, n6, None, n8], bn=[bn_n, bn0, bn1, bn2], f=[f1, f2],
                 pooled=head_in, pmean=pmean, psd=psd, H1=H1, H2=H2, logp=logp_all, head_plan=plan,
                 dims=(B, T, Ltot, L2, L4, La, Lb, Lc), train=train, W=W, A=A, gc=gc, fused_head=fused_head)
        ctx.S, ctx.model, ctx.names, ctx.params = S, model, names, params
        ctx.need_input_grad = feats.requires_grad
        return recon.view(B, T, 80), logp

    @staticmethod
    def backward(ctx, d_recon, d_logp):
        S, model, names = ctx.S, ctx.model, ctx.names
        if S is None:
            raise SaHipError("ConvAutoencoder backward called twice (saved tensors were released)")
        P = dict(zip(names, ctx.params))
        dt = model.act_dtype
        B, T, Ltot, L2, L4, La, Lb, Lc = S["dims"]
        if not S["train"]:
            raise SaHipError("backward through eval-mode BatchNorm is not implemented")
        y0, y1, y2, y3, y4, y5, y6, y7, y8 = S["y"]
        r0, r1, r2 = S["r"]
        n1, n2, n3, n4, n6, n8 = S["n"][1], S["n"][2], S["n"][3], S["n"][4], S["n"][6], S["n"][8]
        bn_n, bn0, bn1, bn2 = S["bn"]
        f1, f2 = S["f"]
        dev = y0.device
        G = {k: None for k in names}
        need = {k: p.requires_grad for k, p in P.items()}
        # which stages have anything to produce (the epoch-parity schedule of the reference freezes
        # either the classifier or everything else, speechbrain_convae_train.py:212-235): like
        # autograd in the reference, nothing is computed below the last tensor that needs a gradient
        need_stage = {st: any(v for k, v in need.items() if k.startswith(st))
                      for st in sdist.StageBuckets.STAGES}
        run_encoder = need_stage["encoder"] or ctx.need_input_grad
        run_decoder = need_stage["decoder"] or run_encoder
        # the buckets of an earlier backward must not outlive it (Brain._grad_flats would match them against this
        # step's .grad, and they would stay pinned -- in the graph pool under hipGraph): finish() sets the new ones
        model._last_flats = None
        buckets = sdist.StageBuckets(list(P.items()), dev, model._side_stream(dev))
        newg = buckets.view

        def setg(key, val):
            G[key] = newg(key).copy_(val.reshape(P[key].shape))
        W, A, lay = S["W"], S["A"], model.lay
        gc = S["gc"]                                      # all-reduced BatchNorm counts (or None)
        cdev = lambda i: None if gc is None else gc[i:i + 1]
        # the split-K reducers of a stage's weight gradients wait for the end of the stage like the bias
        # gradients (nobody reads them earlier) and run as one launch (sa_wgrad_reduce_multi)
        pending_wred = []
        wg = functools.partial(ops.wgrad, code=ops.WGRAD_CODE[model.precision], defer=pending_wred)
        # with the bf16 operand caches in place the apply pass of every normalised layer whose
        # gradient feeds a convolution moves into that convolution's prologue
        fuse = bool(A) and model.dgrad_kcode in (L.BF16X3, L.BF16)

        def cg(ly, gin, **kw):
            """the layer's data-gradient launch; a _PendingApply input selects the
            normalisation-backward prologue, which also emits the bf16 d y for the deferred weight
            gradients and the column sums for the bias gradient."""
            p, dy = gin, gin.g if isinstance(gin, _PendingApply) else gin
            w, args = W[ly.key, ly.kinds[1]], (None,) + ly.dgrad(ly.lin(dy.shape[1]))
            if dy is gin:
                return _conv(dy, w, *args, **kw)
            dyc = torch.empty(p.g.shape, dtype=torch.bfloat16, device=p.g.device) if p.wgrads else None
            want_cs = p.bias_key is not None and need[p.bias_key]
            out = _conv(p.g, w, *args, a_out=dyc, nb=dict(x=p.y, c1=p.c[0], c2=p.c[1], c3=p.c[2],
                                                           per_c=p.per_c, relu_mask=p.relu,
                                                           want_colsum=want_cs), **kw)
            if want_cs:
                cs = out[-1]
                out = out[:-1] if len(out) > 2 else out[0]
                nb_, _, cc_ = cs.shape
                G[p.bias_key] = newg(p.bias_key)
                pending_bias.append((cs, nb_, cc_, 1, G[p.bias_key]))
            for f in p.wgrads:
                f(dyc)
            p.wgrads = []
            return out

        def bias_from(stats, key, C):
            if need[key]:
                G[key] = newg(key)
                pending_bias.append((stats, B, C, 2, G[key]))

        # bias gradients wait for the end of their stage: nothing reads them before the stage's
        # bucket is reduced, so all of a stage's slab sums run as two launches (sa_bias_multi)
        pending_bias = []

        def flush_pending():
            """the stage's queued bias sums, then its queued split-K reducers"""
            if pending_bias:
                ops.bias_multi(pending_bias)
                pending_bias.clear()
            if pending_wred:
                ops.wgrad_reduce_multi(pending_wred)
                pending_wred.clear()

        def in_finish(g, st, y, nrm, C, Ln, prefix, bias_key):
            """g = d z (already multiplied by swish'), st = partial (sum dz, sum dz*yhat)."""
            mean, rstd = nrm[0], nrm[1]
            dg, db = newg(prefix + ".weight"), newg(prefix + ".bias")
            sums = ops.sum_partials(st, B)
            c1, c2, c3 = ops.fin_norm_bwd(sums, sums, B * C, C, Ln, P[prefix + ".weight"], mean, rstd,
                                          dgamma=dg, dbeta=db)
            G[prefix + ".weight"], G[prefix + ".bias"] = dg, db
            if fuse:
                return _PendingApply(g, y, (c1, c2, c3), False, False, bias_key)
            st2 = ops.ew("apply", g, y, C, out=g, c1=c1, c2=c2, c3=c3)
            bias_from(st2, bias_key, C)
            return g                                             # now d y

        def bn_ep(r, bn, xp=None):
            d = dict(mode=2, x=r, mean=bn[0], rstd=bn[1], per_c=True)
            if xp:
                d.update(s1=xp[0], t1=xp[1], xp_is_act=True)
            return d

        def bn_finish(g, st, r, bn, Ln, prefix, bias_key, ci, xp=None):
            """backward of [conv -> ReLU -> BatchNorm(prefix)] w.r.t. the conv output (stored r =
            relu output); xp=(s1,t1): the BN input is swish(r*s1+t1) instead (the `norm` BN on the
            encoder output, with GradReverse in front: sign -1, no ReLU mask)."""
            mean, rstd = bn[0], bn[1]
            kw = dict(s1=xp[0], t1=xp[1], xp_is_act=True) if xp else {}
            dg, db = newg(prefix + ".weight"), newg(prefix + ".bias")
            lsums = ops.sum_partials(st, 1, rows=model._bn_rows())
            gsums, _ = model._bn_global(lsums)
            c1, c2, c3 = ops.fin_norm_bwd(gsums, lsums, 128, 128, float(B * Ln), P[prefix + ".weight"],
                                          mean, rstd, sign=-1.0 if xp else 1.0, dgamma=dg, dbeta=db,
                                          n_dev=cdev(ci))
            G[prefix + ".weight"], G[prefix + ".bias"] = dg, db
            if fuse:
                return _PendingApply(g, r, (c1, c2, c3), True, not xp, bias_key)
            st2 = ops.ew("apply", g, r, 128, out=g, c1=c1, c2=c2, c3=c3, relu_mask=not xp, per_c=True,
                         want_stats=bias_key is not None, **kw)
            if bias_key:
                bias_from(st2, bias_key, 128)
            return g

        def conv_wgrad(ly, x, dy, **pro):
            key = ly.key
            if not need[key]:
                return
            if isinstance(dy, _PendingApply):                # runs once the bf16 d y exists
                dy.wgrads.append(lambda dyc: conv_wgrad(ly, x, dyc, dy_pre=True))
                return
            if key in A:
                x, pro = A[key], dict(x_pre=True, dy_pre=bool(pro.get("dy_pre")))
            *geo, strides = ly.wgrad(x.shape[1])
            G[key] = wg(x, dy, *geo, newg(key), strides, **pro)

        # an output the loss does not use (the endtoend "sex only" branch,
        # speechbrain_convae_train.py:112-113, leaves recon out of the graph): like autograd in the
        # reference, the parameters that only feed that output get NO gradient (None, so that Adam
        # skips them) rather than zeros
        recon_unused = d_recon is None
        if recon_unused:
            for k in need:
                if k.startswith("decoder"):
                    need[k] = False
            need_stage["decoder"] = False
        if d_logp is None:
            d_logp = torch.zeros(B, 2, device=dev)

        def finish(d_feats=None):
            flush_pending()
            buckets.join()
            ctx.S = None
            # (Brain.check_gradients clips the buckets directly when every .grad is still a view of one of them):
            # the stages with anything to produce are the ones reduced on every return path
            model._last_flats = [buckets.flat[st] for st in sdist.StageBuckets.STAGES if need_stage[st]]
            grads = tuple(G[k] if need[k] else None for k in names)
            G.clear()
            buckets.views.clear()
            return (None, None, d_feats) + grads

        # ======================= sex classifier: FC head =======================
        def head_bwd():
            c = "sex_classifier.classify."
            plan = S.get("head_plan")
            dlp, Bh = d_logp.contiguous().float(), B
            if plan:                                  # d log p of every rank's rows, one exchange
                dlp, Bh = model._gather_rows(dlp, plan), plan[1]
            dP = head_bwd_rows(c, dlp, Bh, plan is not None)
            if plan:
                # every rank now holds the head gradients of the SUM of the ranks' losses; the
                # data-parallel average that follows expects each rank's share
                hg = [G[k] for k in names if k.startswith(c) and k in G]
                if plan[2] > 1 and hg:
                    torch._foreach_mul_(hg, 1.0 / plan[2])
                dP = dP[plan[0]:plan[0] + B]
            return dP

        def head_bwd_rows(c, dlp, n, local):
            if S.get("fused_head"):                  # the whole chain in one launch (sa_head_bwd)
                short = ("0.weight", "0.bias", "2.weight", "2.bias", "3.weight", "3.bias", "5.weight", "5.bias",
                         "6.weight", "6.bias")
                views = {}
                for k in short:
                    if need[c + k]:
                        views[k] = G[c + k] = newg(c + k)
                clsP = {k: P[c + k] for k in short}
                return ops.head_bwd(dlp, S["logp"], S["pooled"], S["H1"], f1, S["H2"], f2, clsP, views,
                                    wide=model.wide_head_bwd)
            glob = (lambda l: l) if local else (lambda l: model._bn_global(l)[0])
            cd = (lambda i: None) if local else cdev
            dLG = ops.log_softmax_bwd(dlp, S["logp"])
            H1, H2 = S["H1"], S["H2"]
            G[c + "6.weight"] = ops.dense_wgrad(dLG, H2, newg(c + "6.weight"), ps=f2[2], pt=f2[3])
            G[c + "6.bias"] = newg(c + "6.bias"); ops.colsums(dLG, out0=G[c + "6.bias"])
            dN2 = ops.dense(dLG, P[c + "6.weight"], None, 64, 2, transpose_w=True)
            G[c + "5.weight"], G[c + "5.bias"] = newg(c + "5.weight"), newg(c + "5.bias")
            l2 = ops.colsums(dN2, H2, f2[0], f2[1], out0=G[c + "5.bias"], out1=G[c + "5.weight"])
            dH2 = ops.bn2d_bwd(dN2, H2, glob(l2), n, P[c + "5.weight"], f2[0], f2[1], True, count_dev=cd(5))
            G[c + "3.weight"] = ops.dense_wgrad(dH2, H1, newg(c + "3.weight"), ps=f1[2], pt=f1[3])
            G[c + "3.bias"] = newg(c + "3.bias"); ops.colsums(dH2, out0=G[c + "3.bias"])
            dN1 = ops.dense(dH2, P[c + "3.weight"], None, 128, 64, transpose_w=True)
            G[c + "2.weight"], G[c + "2.bias"] = newg(c + "2.weight"), newg(c + "2.bias")
            l1 = ops.colsums(dN1, H1, f1[0], f1[1], out0=G[c + "2.bias"], out1=G[c + "2.weight"])
            dH1 = ops.bn2d_bwd(dN1, H1, glob(l1), n, P[c + "2.weight"], f1[0], f1[1], True, count_dev=cd(4))
            G[c + "0.weight"] = ops.dense_wgrad(dH1, S["pooled"], newg(c + "0.weight"))
            G[c + "0.bias"] = newg(c + "0.bias"); ops.colsums(dH1, out0=G[c + "0.bias"])
            return ops.dense(dH1, P[c + "0.weight"], None, 256, 128, transpose_w=True)

        # ======================= sex classifier: pooling + TDNN (its input gradient is an addend
        # of the encoder-output gradient that the last decoder dgrad fuses in) =======================
        def tdnn_bwd(dP):
            t = "sex_classifier.tdnn."
            g, st = ops.pool_bwd(r2, bn2[2], bn2[3], dP, S["pmean"], S["psd"], bn=(bn2[0], bn2[1]))
            g = bn_finish(g, st, r2, bn2, Lc, t + "8", t + "6.bias", 3)
            conv_wgrad(lay[t + "6"], r1, g, s2=bn1[2], t2=bn1[3])
            g, st = cg(lay[t + "6"], g, want_stats=True, ep=bn_ep(r1, bn1))
            g = bn_finish(g, st, r1, bn1, Lb, t + "5", t + "3.bias", 2)
            conv_wgrad(lay[t + "3"], r0, g, s2=bn0[2], t2=bn0[3])
            g, st = cg(lay[t + "3"], g, want_stats=True, ep=bn_ep(r0, bn0))
            g = bn_finish(g, st, r0, bn0, La, t + "2", t + "0.bias", 1)
            conv_wgrad(lay[t + "0"], y4, g, s1=n4[2], t1=n4[3], swish=True, s2=bn_n[2], t2=bn_n[3])
            xp4 = (n4[2], n4[3])
            g, st = cg(lay[t + "0"], g, want_stats=True, ep=bn_ep(y4, bn_n, xp4))
            da = bn_finish(g, st, y4, bn_n, L4, "sex_classifier.norm", None, 0, xp=xp4)      # includes GRL
            flush_pending()
            if need_stage["sex_classifier"]:
                buckets.reduce_stage("sex_classifier")
            return da

        # ======================= decoder =======================
        def decoder_bwd():
            d_rec = torch.zeros(B, T, 80, device=dev) if recon_unused else d_recon
            g_rec = d_rec.reshape(B, Ltot).contiguous().float()
            if need["decoder.8.bias"]:
                setg("decoder.8.bias", ops.sum_partials(g_rec.view(4 * B, Ltot // 4), 1, n=Ltot // 4).sum())
            if need["decoder.8.weight"] and model.fused_bwd1c:
                g, st, G["decoder.8.weight"] = ops.bwd1C(g_rec, y8, P["decoder.8.weight"], newg("decoder.8.weight"),
                                                         n8[2], n8[3], n8[0], n8[1])             # d z8
            else:
                if need["decoder.8.weight"]:
                    G["decoder.8.weight"] = ops.wgrad1C(g_rec, y8, newg("decoder.8.weight"), flip=True,
                                                        s1=n8[2], t1=n8[3], swish=True)
                g, st = ops.conv1toC(g_rec, P["decoder.8.weight"], None, dt, flip=True, want_stats=True,
                                     ep=dict(x=y8, s1=n8[2], t1=n8[3], mean=n8[0], rstd=n8[1]))  # d z8
            g = in_finish(g, st, y8, n8, 32, Ltot, "decoder.6", "decoder.5.bias")               # d y8
            conv_wgrad(lay["decoder.5"], y7, g)
            g, st = cg(lay["decoder.5"], g, want_stats=True)                                    # d y7
            bias_from(st, "decoder.4.bias", 64)
            conv_wgrad(lay["decoder.4"], y6, g, s1=n6[2], t1=n6[3], swish=True)
            g, st = cg(lay["decoder.4"], g, want_stats=True, ep=_in_ep(y6, n6))                 # d z6
            g = in_finish(g, st, y6, n6, 64, L2, "decoder.2", "decoder.1.bias")                 # d y6
            conv_wgrad(lay["decoder.1"], y5, g)
            g, st = cg(lay["decoder.1"], g, want_stats=True)                                    # d y5
            bias_from(st, "decoder.0.bias", 128)
            conv_wgrad(lay["decoder.0"], y4, g, s1=n4[2], t1=n4[3], swish=True)
            flush_pending()
            if need_stage["decoder"]:
                buckets.reduce_stage("decoder")
            return g

        da4_cls = tdnn_bwd(head_bwd())
        if not run_decoder:                       # classifier-only step: nothing below needs a gradient
            return finish()
        g = decoder_bwd()
        if not run_encoder:
            return finish()

        # ======================= encoder =======================
        # d z4 = (decoder.0 dgrad + classifier branch) * swish'(z4), fused into the dgrad launch
        g, st = cg(lay["decoder.0"], g, want_stats=True, ep=_in_ep(y4, n4, g2=da4_cls))
        # per layer: y = conv(swish(nx(x))) and nrm the InstanceNorm on y; encoder.2's input y0 carries no norm
        for conv, norm, y, nrm, x, nx in (("encoder.11", "encoder.12", y4, n4, y3, n3),
                                          ("encoder.8", "encoder.9", y3, n3, y2, n2),
                                          ("encoder.5", "encoder.6", y2, n2, y1, n1),
                                          ("encoder.2", "encoder.3", y1, n1, y0, None)):
            ly = lay[conv]
            g = in_finish(g, st, y, nrm, ly.cout, y.shape[1], norm, ly.bias)                    # d y
            conv_wgrad(ly, x, g, swish=True, **(dict(s1=nx[2], t1=nx[3]) if nx else {}))
            g, st = cg(ly, g, want_stats=True, ep=_in_ep(x, nx) if nx else dict(mode=1, x=x))   # d z below (d y0 last)
        bias_from(st, "encoder.0.bias", 32)
        if need["encoder.0.weight"]:
            G["encoder.0.weight"] = ops.wgrad1C(S["x0"], g, newg("encoder.0.weight"))
        d_feats = None
        if ctx.need_input_grad:
            d_feats = ops.convCto1(g, P["encoder.0.weight"], None, flip=True).view(B, T, 80)
        flush_pending()
        if need_stage["encoder"]:
            buckets.reduce_stage("encoder")
        # autograd's AccumulateGrad adopts a gradient only when nothing else references it (it
        # clones otherwise: 56 copies per step): finish() drops this frame's references explicitly
        # rather than rely on the frame being collected before the engine looks
        return finish(d_feats)
