"""FullyConnectedAutoencoder: drop-in for ``models.FullyConnected.FullyConnectedAutoencoder`` of the
reference (models/FullyConnected.py:65-104,118-159; ``--model_type fcae``) with the whole forward and
backward on libsa_hip.so (csrc/sa_fcae.hip), fp32 throughout.

Same constructor ``(mfcc_feature_dim, batch_size)``, same ``forward(feats[B,T,80]) -> (recon[B,T,80],
log_probs[B,2])``, same parameter / buffer names (``encoder.0.weight`` ... ``sex_classifier.classify.7.bias``).
The torch.nn layers are parameter containers only; one ``torch.autograd.Function`` runs the nine launches
(DESIGN section 10):

  forward   enc_fwd -> bn_fin -> mid_fwd -> head_fwd
  backward  head_bwd -> mid_bwd -> bn_bwd_fin -> enc_bwd -> wreduce

The functions of this module with those names are the launches themselves (one library call each); the
tests check each of them against fp64 formulas.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import SaHipError

FRAME_LAYERS = ("encoder.0", "encoder.2", "encoder.4", "decoder.0", "decoder.2", "decoder.4",
                "sex_classifier.initial.0", "sex_classifier.initial.2")
FRAME_DIMS = ((60, 80), (40, 60), (20, 40), (40, 20), (60, 40), (80, 60), (40, 20), (40, 40))
_CL = "sex_classifier.classify."
# the order of sa_fc_head_fwd's pointer table
HEAD_PTRS = ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var", "3.weight", "3.bias",
             "5.weight", "5.bias", "6.weight", "6.bias", "6.running_mean", "6.running_var", "7.weight", "7.bias")
# the order of sa_fc_head_bwd's gradient record
HEAD_GRADS = (("0.weight", (40, 80)), ("0.bias", (40,)), ("1.weight", (40,)), ("1.bias", (40,)),
              ("3.weight", (40, 40)), ("3.bias", (40,)), ("5.weight", (20, 40)), ("5.bias", (20,)),
              ("6.weight", (20,)), ("6.bias", (20,)), ("7.weight", (2, 20)), ("7.bias", (2,)))
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


class _ParamOnly(nn.Module):
    """keeps the Sequential indices of the reference."""

    def forward(self, x):                                        # pragma: no cover
        raise SaHipError("parameter container only; use FullyConnectedAutoencoder.forward")


class ReLU(_ParamOnly):
    pass


class StatisticsPooling(_ParamOnly):
    pass


class FullyConnSexClassifier(nn.Module):
    def __init__(self, num_classes=2):
        super().__init__()
        self.initial = nn.Sequential(nn.Linear(20, 40), ReLU(), nn.Linear(40, 40), ReLU())
        self.norm = nn.BatchNorm1d(20)
        self.classify = nn.Sequential(
            nn.Linear(80, 40), nn.BatchNorm1d(40), ReLU(), nn.Linear(40, 40), ReLU(), nn.Linear(40, 20),
            nn.BatchNorm1d(20), nn.Linear(20, num_classes))
        self.stats_pooling = StatisticsPooling()

    def forward(self, x):                                        # pragma: no cover
        raise SaHipError("parameter container only; use FullyConnectedAutoencoder.forward")


# ---------------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------------
def _f32(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise SaHipError(f"{what}: the fcae kernels take GPU tensors (no CPU fallback)")
    if t.dtype != torch.float32:
        raise SaHipError(f"{what}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise SaHipError(f"{what}: expected a contiguous tensor")
    if t.data_ptr() % 16:
        raise SaHipError(f"{what}: expected 16-byte aligned storage")
    return t


def _table(tensors, what):
    """host array of device pointers (the library copies it into the kernel arguments)"""
    return (C.c_void_p * len(tensors))(*[_f32(t, what).data_ptr() for t in tensors])


def frame_table(P):
    """P: name -> tensor of the eight per-frame Linears (FRAME_LAYERS)"""
    ws = [P[k + ".weight"] for k in FRAME_LAYERS] + [P[k + ".bias"] for k in FRAME_LAYERS]
    for t, (n, k) in zip(ws[:8], FRAME_DIMS):
        if tuple(t.shape) != (n, k):
            raise SaHipError(f"fcae: weight of shape {tuple(t.shape)} where [{n}, {k}] is expected")
    return _table(ws, "fcae parameter")


def head_table(H):
    """H: name -> tensor of classify's parameters and running statistics (HEAD_PTRS)"""
    return _table([H[k] for k in HEAD_PTRS], "fcae classify parameter")


def _bt(feats):
    B, T, Fd = feats.shape
    if Fd != 80 or T < 2:
        raise SaHipError("fcae expects feats [B, T, 80] with T >= 2")
    return B, T


def max_rows():
    return L.load().sa_fc_max_rows()


def groups(B, T):
    return L.load().sa_fc_groups(B, T)


def tiles(T):
    return L.load().sa_fc_tiles(T)


def enc_fwd(feats, wb):
    """-> h1 [B,T,60], h2 [B,T,40], z [B,T,20], bnpart [B*tiles,20,2] (fp64)"""
    lib = L.load()
    B, T = _bt(_f32(feats, "feats"))
    e = lambda c: torch.empty(B, T, c, device=feats.device)
    h1, h2, z = e(60), e(40), e(20)
    bnpart = torch.empty(B * tiles(T), 20, 2, dtype=torch.float64, device=feats.device)
    L.check(lib.sa_fc_enc_fwd(L.ptr(feats), wb, L.ptr(h1), L.ptr(h2), L.ptr(z), L.ptr(bnpart), B, T, L.stream()),
            "sa_fc_enc_fwd")
    return h1, h2, z, bnpart


def bn_fin(bnpart, norm_w, norm_b, run_mean, run_var, B, T, train):
    """-> bnf [4,20] (mean, rstd, scale, shift); train: updates run_mean / run_var in place"""
    lib = L.load()
    bnf = torch.empty(4, 20, device=norm_w.device)
    L.check(lib.sa_fc_bn_fin(L.ptr(bnpart), 0 if bnpart is None else bnpart.shape[0], L.ptr(_f32(norm_w, "norm.weight")),
                             L.ptr(_f32(norm_b, "norm.bias")), L.ptr(_f32(run_mean, "norm.running_mean")),
                             L.ptr(_f32(run_var, "norm.running_var")), L.ptr(bnf), B, T, int(train),
                             C.c_float(BN_EPS), C.c_float(BN_MOMENTUM), L.stream()), "sa_fc_bn_fin")
    return bnf


def mid_fwd(z, bnf, wb):
    """-> a1, u [B,T,40], d1 [B,T,40], d2 [B,T,60], recon [B,T,80], poolpart [B*tiles,2,40] (fp64)"""
    lib = L.load()
    B, T, _ = _f32(z, "z").shape
    e = lambda c: torch.empty(B, T, c, device=z.device)
    a1, u, d1, d2, recon = e(40), e(40), e(40), e(60), e(80)
    poolpart = torch.empty(B * tiles(T), 2, 40, dtype=torch.float64, device=z.device)
    L.check(lib.sa_fc_mid_fwd(L.ptr(z), L.ptr(_f32(bnf, "bnf")), wb, L.ptr(a1), L.ptr(u), L.ptr(d1), L.ptr(d2),
                              L.ptr(recon), L.ptr(poolpart), B, T, L.stream()), "sa_fc_mid_fwd")
    return a1, u, d1, d2, recon, poolpart


def recon_fwd(feats, wb):
    """feats [B,T,80] -> recon [B,T,80] = decoder(encoder(feats)), one launch, nothing else stored; the bits of
    mid_fwd's recon.  Any B >= 1 and T >= 1 (no pooling, no head)."""
    lib = L.load()
    B, T, Fd = _f32(feats, "feats").shape
    if Fd != 80 or T < 1 or B < 1:
        raise SaHipError("fcae expects feats [B, T, 80] with B >= 1 and T >= 1")
    recon = torch.empty(B, T, 80, device=feats.device)
    L.check(lib.sa_fc_recon_fwd(L.ptr(feats), wb, L.ptr(recon), B, T, L.stream()), "sa_fc_recon_fwd")
    return recon


def _rows_ok(B):
    if B > max_rows():
        raise SaHipError(f"fcae: the classifier head runs as one workgroup of at most {max_rows()} utterances, "
                         f"got a batch of {B}")


def head_fwd(poolpart, noise, hw, B, T, train):
    """-> dict(pooled [B,80], pst [B,80], h1 [B,40], f1 [4,40], h2 [B,40], h3 [B,20], f2 [4,20], logp [B,2]);
    train: updates the running statistics of classify.1 / classify.6 in place"""
    lib = L.load()
    _rows_ok(B)
    if train and B < 2:
        raise SaHipError("fcae: BatchNorm1d in train mode needs more than one utterance per batch")
    dev = poolpart.device
    e = lambda *s: torch.empty(*s, device=dev)
    o = dict(pooled=e(B, 80), pst=e(B, 80), h1=e(B, 40), f1=e(4, 40), h2=e(B, 40), h3=e(B, 20), f2=e(4, 20),
             logp=e(B, 2))
    if noise is not None and tuple(_f32(noise, "pooling noise").shape) != (B, 40):
        raise SaHipError(f"fcae: pooling noise must be [{B}, 40]")
    L.check(lib.sa_fc_head_fwd(L.ptr(poolpart), L.ptr(noise), hw, L.ptr(o["pooled"]), L.ptr(o["pst"]), L.ptr(o["h1"]),
                               L.ptr(o["f1"]), L.ptr(o["h2"]), L.ptr(o["h3"]), L.ptr(o["f2"]), L.ptr(o["logp"]), B, T,
                               int(train), C.c_float(BN_EPS), C.c_float(BN_MOMENTUM), L.stream()), "sa_fc_head_fwd")
    return o


def head_bwd(dlogp, o, hw, train, dhead=None):
    """dlogp [B,2], o: head_fwd's outputs -> dhead [5862] (HEAD_GRADS order), dpooled [B,80]"""
    lib = L.load()
    B = _f32(dlogp, "d logp").shape[0]
    _rows_ok(B)
    if dhead is None:
        dhead = torch.empty(lib.sa_fc_nhead(), device=dlogp.device)
    dpooled = torch.empty(B, 80, device=dlogp.device)
    L.check(lib.sa_fc_head_bwd(L.ptr(dlogp), L.ptr(o["logp"]), L.ptr(o["pooled"]), L.ptr(o["h1"]), L.ptr(o["h2"]),
                               L.ptr(o["h3"]), hw, L.ptr(dhead), L.ptr(dpooled), B,
                               int(train), C.c_float(BN_EPS), L.stream()), "sa_fc_head_bwd")
    return dhead, dpooled


def split_head_grads(dhead):
    out, o = {}, 0
    for k, shp in HEAD_GRADS:
        n = 1
        for s in shp:
            n *= s
        out[k] = dhead[o:o + n].view(shp)
        o += n
    return out


def mid_bwd(d_recon, dpooled, pst, z, bnf, a1, u, d1, d2, wb, wpart=None):
    """-> dzn, dzdec [B,T,20], wpart [G,nparam] (decoder / initial slices written), bnbpart [G,20,2] (fp64)"""
    lib = L.load()
    B, T = _bt(_f32(d_recon, "d recon"))
    G = groups(B, T)
    dev = z.device
    dzn, dzdec = torch.empty(B, T, 20, device=dev), torch.empty(B, T, 20, device=dev)
    if wpart is None:
        wpart = torch.empty(G, lib.sa_fc_nparam(), device=dev)
    bnbpart = torch.empty(G, 20, 2, dtype=torch.float64, device=dev)
    L.check(lib.sa_fc_mid_bwd(L.ptr(d_recon), L.ptr(_f32(dpooled, "d pooled")), L.ptr(pst), L.ptr(z), L.ptr(bnf),
                              L.ptr(a1), L.ptr(u), L.ptr(d1), L.ptr(d2), wb, L.ptr(dzn), L.ptr(dzdec), L.ptr(wpart),
                              L.ptr(bnbpart), B, T, L.stream()), "sa_fc_mid_bwd")
    return dzn, dzdec, wpart, bnbpart


def bn_bwd_fin(bnbpart, norm_w, bnf, B, T, train, dgamma=None, dbeta=None):
    """-> coef [3,20] of d z = c1 dzn + c2 z + c3 (GradReverse folded in), d norm.weight, d norm.bias"""
    lib = L.load()
    dev = bnf.device
    coef = torch.empty(3, 20, device=dev)
    dgamma = torch.empty(20, device=dev) if dgamma is None else dgamma
    dbeta = torch.empty(20, device=dev) if dbeta is None else dbeta
    L.check(lib.sa_fc_bn_bwd_fin(L.ptr(bnbpart), bnbpart.shape[0], L.ptr(_f32(norm_w, "norm.weight")), L.ptr(bnf),
                                 L.ptr(coef), L.ptr(dgamma), L.ptr(dbeta), B, T, int(train), L.stream()),
            "sa_fc_bn_bwd_fin")
    return coef, dgamma, dbeta


def enc_bwd(feats, h1, h2, z, dzn, dzdec, coef, wb, wpart):
    """writes the encoder slices of wpart [G,nparam]"""
    lib = L.load()
    B, T = _bt(_f32(feats, "feats"))
    if tuple(wpart.shape) != (groups(B, T), lib.sa_fc_nparam()):
        raise SaHipError("fcae: wpart must be [sa_fc_groups(B, T), sa_fc_nparam()]")
    L.check(lib.sa_fc_enc_bwd(L.ptr(feats), L.ptr(h1), L.ptr(h2), L.ptr(z), L.ptr(dzn), L.ptr(dzdec), L.ptr(coef), wb,
                              L.ptr(wpart), B, T, L.stream()), "sa_fc_enc_bwd")
    return wpart


def wreduce(wpart, grads=None):
    """-> grads [nparam]: the eight weight gradients (nn.Linear layout), then the eight bias gradients"""
    lib = L.load()
    if grads is None:
        grads = torch.empty(lib.sa_fc_nparam(), device=wpart.device)
    L.check(lib.sa_fc_wreduce(L.ptr(_f32(wpart, "wpart")), wpart.shape[0], L.ptr(grads), L.stream()), "sa_fc_wreduce")
    return grads


def split_frame_grads(grads):
    out, o = {}, 0
    for k, (n, kk) in zip(FRAME_LAYERS, FRAME_DIMS):
        out[k + ".weight"] = grads[o:o + n * kk].view(n, kk)
        o += n * kk
    for k, (n, _) in zip(FRAME_LAYERS, FRAME_DIMS):
        out[k + ".bias"] = grads[o:o + n]
        o += n
    return out


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
def _noise(model, B, device):
    """convae.ConvAutoencoder.pooling_noise's conventions: False / None -> off, True -> speechbrain's draw,
    a tensor [B, 40] in [0, 1] -> that draw"""
    n = model.pooling_noise
    if n is None or n is False:
        return None
    if torch.is_tensor(n):
        return n.to(device=device, dtype=torch.float32).contiguous()
    g = torch.randn(B, 40, device=device)                       # speechbrain _get_gauss_noise
    g = g - g.min()
    return (g / g.max()).contiguous()


class _FcAEFn(torch.autograd.Function):
    """(recon, logp) = f(feats; 30 parameters).  There is NO gradient to ``feats``: backward returns None
    for it (the model is the first differentiable stage of every caller; the features come from the
    Fbank / normaliser, which have no parameters)."""

    @staticmethod
    def forward(ctx, model, names, feats, *params):
        if not torch.is_tensor(feats) or not feats.is_cuda:
            raise SaHipError("FullyConnectedAutoencoder runs on the GPU only (no CPU fallback)")
        if feats.dim() != 3:
            raise SaHipError("fcae expects feats [B, T, 80]")
        feats = _f32(feats.detach(), "feats")
        B, T = _bt(feats)
        P = dict(zip(names, params))
        cls = model.sex_classifier
        train = model.training
        wb = frame_table(P)
        H = {k[len(_CL):]: v for k, v in P.items() if k.startswith(_CL)}
        for i in (1, 6):
            H[f"{i}.running_mean"], H[f"{i}.running_var"] = cls.classify[i].running_mean, cls.classify[i].running_var
        hw = head_table(H)
        _rows_ok(B)
        h1, h2, z, bnpart = enc_fwd(feats, wb)
        bnf = bn_fin(bnpart if train else None, P["sex_classifier.norm.weight"], P["sex_classifier.norm.bias"],
                     cls.norm.running_mean, cls.norm.running_var, B, T, train)
        a1, u, d1, d2, recon, poolpart = mid_fwd(z, bnf, wb)
        o = head_fwd(poolpart, _noise(model, B, feats.device), hw, B, T, train)
        if train:
            torch._foreach_add_([cls.norm.num_batches_tracked, cls.classify[1].num_batches_tracked,
                                 cls.classify[6].num_batches_tracked], 1)
        if any(ctx.needs_input_grad):
            ctx.S = dict(feats=feats, h1=h1, h2=h2, z=z, bnf=bnf, a1=a1, u=u, d1=d1, d2=d2, head=o, wb=wb, hw=hw,
                         P=P, train=train, dims=(B, T))
            ctx.model, ctx.names = model, names
        return recon, o["logp"]

    @staticmethod
    def backward(ctx, d_recon, d_logp):
        S, model, names = ctx.S, ctx.model, ctx.names
        B, T = S["dims"]
        P, wb, hw, o, train = S["P"], S["wb"], S["hw"], S["head"], S["train"]
        lib = L.load()
        dev = S["z"].device
        np_, nh = lib.sa_fc_nparam(), lib.sa_fc_nhead()
        # every gradient of the step is a view of this one buffer: frame Linears | classify | norm
        flat = torch.empty(np_ + nh + 40, device=dev)
        dhead, dpooled = head_bwd(d_logp.contiguous(), o, hw, train, flat[np_:np_ + nh])
        dzn, dzdec, wpart, bnbpart = mid_bwd(d_recon.contiguous(), dpooled, o["pst"], S["z"], S["bnf"], S["a1"], S["u"],
                                             S["d1"], S["d2"], wb)
        coef, dgamma, dbeta = bn_bwd_fin(bnbpart, P["sex_classifier.norm.weight"], S["bnf"], B, T, train,
                                         flat[np_ + nh:np_ + nh + 20], flat[np_ + nh + 20:])
        enc_bwd(S["feats"], S["h1"], S["h2"], S["z"], dzn, dzdec, coef, wb, wpart)
        wreduce(wpart, flat[:np_])
        G = split_frame_grads(flat[:np_])
        G.update({_CL + k: v for k, v in split_head_grads(dhead).items()})
        G["sex_classifier.norm.weight"], G["sex_classifier.norm.bias"] = dgamma, dbeta
        grads = [G[n] if need else None for n, need in zip(names, ctx.needs_input_grad[3:])]
        # Brain.check_gradients clips on this buffer when every gradient it sees lives here
        model._last_flats = [flat] if all(g is not None for g in grads) else None
        ctx.S = None
        return (None, None, None, *grads)


class FullyConnectedAutoencoder(nn.Module):
    def __init__(self, mfcc_feature_dim=80, batch_size=None, pooling_noise=True):
        """pooling_noise: speechbrain's StatisticsPooling adds eps*U[1,9] to the pooled mean on every call
        (train and eval); True reproduces that, a tensor [B, 40] in [0, 1] fixes the draw (tests), False /
        None gives the deterministic form."""
        super().__init__()
        if mfcc_feature_dim != 80:
            raise SaHipError(f"FullyConnectedAutoencoder: the kernels are built for 80 features, got {mfcc_feature_dim}")
        self.mfcc_feature_dim, self.batch_size = mfcc_feature_dim, batch_size
        self.encoder = nn.Sequential(nn.Linear(80, 60), ReLU(), nn.Linear(60, 40), ReLU(), nn.Linear(40, 20))
        self.decoder = nn.Sequential(nn.Linear(20, 40), ReLU(), nn.Linear(40, 60), ReLU(), nn.Linear(60, 80))
        self.sex_classifier = FullyConnSexClassifier(2)
        self.pooling_noise = pooling_noise

    @torch.no_grad()
    def reconstruct(self, feats):
        """recon [B, T, 80] = decoder(encoder(feats)) for inference, one launch (sa_fc_recon_fwd): the bits of
        ``forward(feats)[0]``, in train and eval mode alike (the reconstruction path has no normalisation).
        The classifier branch does not run, so no running statistic moves, nothing is kept for a backward, and
        the head's limits do not apply: any B >= 1 (also B = 1 in train mode, B > sa_fc_max_rows) and T >= 1.
        Refuses what forward refuses (CPU tensors, a feature width other than 80, other dtypes)."""
        if not torch.is_tensor(feats) or not feats.is_cuda:
            raise SaHipError("FullyConnectedAutoencoder runs on the GPU only (no CPU fallback)")
        if feats.dim() != 3:
            raise SaHipError("fcae expects feats [B, T, 80]")
        P = {f"{k}.{s}": getattr(self.get_submodule(k), s).detach() for k in FRAME_LAYERS for s in ("weight", "bias")}
        return recon_fwd(_f32(feats.detach(), "feats"), frame_table(P))

    def forward(self, feats):
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
        return _FcAEFn.apply(self, c[0], feats, *c[1])
