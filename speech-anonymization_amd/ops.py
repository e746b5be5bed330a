"""Thin torch-tensor wrappers over the C ABI (one function per entry point family).

Tensors are device memory handles only; all arithmetic happens in libsa_hip.so on the
current torch stream.  Activations are channels-last [B, L, C] (see include/sa_hip.h).
"""
import collections
import ctypes as C
import functools
import math
import sys

import torch

from . import _lib as L

# ------------------------------------------------------------------------------------
# conv geometry: tap tables of the row-gather GEMM for each kind of layer
# ------------------------------------------------------------------------------------
UP2 = [[(1, 0), (0, 2), (-1, 4)], [(1, 1), (0, 3)]]      # k5 s2 p2 (op1): convT fwd / conv-s2 dgrad


def taps_conv(K, dil, pad):
    """Conv1d forward (any stride via SA): input row = m*SA + k*dil - pad."""
    return [[(k * dil - pad, k) for k in range(K)]]


def taps_conv_dgrad_s1(K, dil, pad):
    """stride-1 Conv1d dgrad: dx[i] = sum_k dy[i + pad - k*dil] W[k]^T."""
    return [[(pad - k * dil, k) for k in range(K)]]


def taps_convT_dgrad(K=5, pad=2):
    """ConvTranspose1d(stride 2) dgrad = stride-2 conv over dy (SA = 2)."""
    return [[(k - pad, k) for k in range(K)]]


CONVT_WG_TAPS = [(1, 0), (1, 1), (0, 0), (0, 1), (-1, 0)]     # k5 s2 p2 (op1) convT wgrad: (input row offset, phase) per tap


class ConvGeom(collections.namedtuple("ConvGeom", "key bias cin cout K stride dil pad transposed kinds")):
    """One conv_gemm layer, read once from its nn.Conv1d / nn.ConvTranspose1d container (ConvGeom.of): the
    arguments of its forward, data-gradient and weight-gradient launches for an input length Lin, its parameter
    keys and its pack kinds (forward, dgrad).  Strided and transposed layers exist for k5 s2 p2 (op1) only.
    The launch tuples are cached per length (bounded: utterance lengths vary from batch to batch)."""
    __slots__ = ()

    @classmethod
    def of(cls, prefix, mod):
        T = isinstance(mod, torch.nn.ConvTranspose1d)
        g = cls(prefix + ".weight", prefix + ".bias", mod.in_channels, mod.out_channels, mod.kernel_size[0],
                mod.stride[0], mod.dilation[0], mod.padding[0], T,
                ("convT_fwd", "convT_dgrad") if T else ("conv_fwd", "conv_dgrad"))
        if (T or g.stride != 1) and (g[4:8] != (5, 2, 1, 2) or (T and mod.output_padding[0] != 1)):
            raise L.SaHipError(f"{prefix}: strided / transposed conv layers are k5 s2 p2 (output_padding 1) only")
        return g

    def lout(self, Lin):
        if self.transposed:
            return 2 * Lin
        return Lin // 2 if self.stride == 2 else Lin + 2 * self.pad - self.dil * (self.K - 1)

    def lin(self, Lout):
        """input length of the layer whose output (or output gradient) has Lout rows"""
        if self.transposed:
            return Lout // 2
        return 2 * Lout if self.stride == 2 else Lout - 2 * self.pad + self.dil * (self.K - 1)

    @functools.lru_cache(maxsize=256)
    def fwd(self, Lin):
        """(cin, cout, sa, u, phases, Lout) of conv_gemm"""
        if self.transposed:
            return self.cin, self.cout, 1, 2, UP2, 2 * Lin
        return self.cin, self.cout, self.stride, 1, taps_conv(self.K, self.dil, self.pad), self.lout(Lin)

    @functools.lru_cache(maxsize=256)
    def dgrad(self, Lin):
        """the same tuple for the data gradient: d y [B, lout(Lin), cout] -> d x [B, Lin, cin]"""
        if self.transposed:
            return self.cout, self.cin, 2, 1, taps_convT_dgrad(), Lin
        if self.stride == 2:
            return self.cout, self.cin, 1, 2, UP2, Lin
        return self.cout, self.cin, 1, 1, taps_conv_dgrad_s1(self.K, self.dil, self.pad), Lin

    @functools.lru_cache(maxsize=256)
    def wgrad(self, Lin):
        """(cin, cout, sa, u, taps, Mrows, dst_strides) of wgrad"""
        if self.transposed:
            return self.cin, self.cout, 1, 2, CONVT_WG_TAPS, Lin, (self.cout * self.K, self.K, 1)
        return (self.cin, self.cout, self.stride, 1, [(k * self.dil - self.pad, 0) for k in range(self.K)],
                self.lout(Lin), (self.K, self.cin * self.K, 1))


def conv_layers(model, roots):
    """{"encoder.8": ConvGeom, ...} of the conv_gemm layers under model.<root>, in module order (the
    single-channel first and last layers have their own kernels: conv1toC / convCto1)"""
    return {f"{r}.{n}": ConvGeom.of(f"{r}.{n}", m) for r in roots for n, m in model.get_submodule(r).named_children()
            if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)) and min(m.in_channels, m.out_channels) > 1}


def _f(t):
    return L.ptr(t)


class _Profile:
    """HIP-event timing of ONE kernel family during bench.py's timed region (the events are
    recorded on the stream the kernel is launched on = torch's current stream)."""

    def __init__(self):
        self.key, self.kinds = None, {}

    def enable(self, key):
        self.key, self.kinds = key, {}

    def start(self, key):
        if key != self.key:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, e0, nbytes, flops, alg_bytes=None, kind=""):
        """nbytes: what the launch is designed to move; alg_bytes: SURVEY 8(d)'s algorithmic
        figure (inputs + outputs once, + the stored tensor a fused backward epilogue re-reads);
        kind: which device kernel served the launch (one family can be served by several)."""
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        k = self.kinds.setdefault(kind, {"ev": [], "bytes": 0, "alg_bytes": 0, "flops": 0})
        k["ev"].append((e0, e1))
        k["bytes"] += nbytes
        k["alg_bytes"] += nbytes if alg_bytes is None else alg_bytes
        k["flops"] += flops

    def collect(self):
        """one record per device kernel of the family, largest total time first"""
        torch.cuda.synchronize()
        out = []
        for kind, k in self.kinds.items():
            out.append({"kernel": kind or self.key, "family": self.key, "launches": len(k["ev"]),
                        "ms": sum(a.elapsed_time(b) for a, b in k["ev"]), "bytes": k["bytes"],
                        "alg_bytes": k["alg_bytes"], "flops": k["flops"]})
        out.sort(key=lambda r: -r["ms"])
        self.key, self.kinds = None, {}
        return out


PROFILE = _Profile()


# precision modes of the MFMA kernels: name -> (activation storage dtype, kernel dtype code)
PRECISIONS = {"f32": (torch.float32, L.F32), "bf16": (torch.bfloat16, L.BF16),
              "bf16x3": (torch.float32, L.BF16X3), "bf16x1f": (torch.float32, L.BF16X1F),
              # fp8: bf16 storage, OCP e4m3 MFMA operands (weights + activations) in the forward
              # convolutions; gradients on the bf16 kernels (BASELINE config 5)
              "fp8": (torch.bfloat16, L.FP8)}
# kernel code of the weight-gradient GEMM per model precision (SA_BF16X1F: see sa_common.h)
WGRAD_CODE = {"f32": L.F32, "bf16": L.BF16, "bf16x3": L.BF16X1F, "bf16x1f": L.BF16X1F, "fp8": L.BF16}
# kernel code of the data-gradient convolutions per model precision
DGRAD_CODE = {"f32": L.F32, "bf16": L.BF16, "bf16x3": L.BF16X3, "bf16x1f": L.BF16X1F, "fp8": L.BF16}


def _pack_geometry(shape, kind):
    """(Kw, K, N, sk, sn) of sa_pack_weights for a parameter of `shape` used as `kind`."""
    if kind in ("conv_fwd", "conv_dgrad"):
        Cout, Cin, Kw = shape
        if kind == "conv_fwd":
            return Kw, Cin, Cout, Kw, Cin * Kw
        return Kw, Cout, Cin, Cin * Kw, Kw
    Cin, Cout, Kw = shape
    if kind == "convT_fwd":
        return Kw, Cin, Cout, Cout * Kw, Kw
    return Kw, Cout, Cin, Kw, Cout * Kw


def _image_buffer(code, dtype, n, device):
    if code == L.FP8:                       # e4m3 image + its per-tensor scale (a float) behind it
        return torch.empty(n + 4, dtype=torch.uint8, device=device)
    if code == L.BF16X3:
        return torch.empty(2 * n, dtype=torch.bfloat16, device=device)
    if code in (L.BF16X1F, L.BF16):
        return torch.empty(n, dtype=torch.bfloat16, device=device)
    return torch.empty(n, dtype=torch.float32, device=device)


def pack_weights(w, kind, dtype, code=None):
    """w: fp32 parameter in PyTorch layout.  kind: conv_fwd | conv_dgrad | convT_fwd |
    convT_dgrad.  Returns the fragment-major operand image (flat tensor; for code BF16X3 the
    hi image followed by the lo image, both bf16)."""
    lib = L.load()
    code = L.dt_code(dtype) if code is None else code
    Kw, K, N, sk, sn = _pack_geometry(w.shape, kind)
    out = _image_buffer(code, dtype, Kw * K * N, w.device)
    L.check(lib.sa_pack_weights(code, _f(w), _f(out), Kw, K, N, sk, sn, 1, L.stream()),
            "sa_pack_weights")
    return out


class PackedWeights:
    """Persistent operand images of a fixed list of (parameter, kind, code) and the device-side
    descriptor table that lets one sa_pack_weights_multi launch refresh all of them."""

    def __init__(self, items, dtype):
        """items: list of (tag, fp32 parameter tensor, kind, code)."""
        self.images, descs = {}, (L.SaPackDesc * len(items))()
        dev = items[0][1].device
        for d, (tag, w, kind, code) in zip(descs, items):
            Kw, K, N, sk, sn = _pack_geometry(w.shape, kind)
            img = _image_buffer(code, dtype, Kw * K * N, dev)
            self.images[tag] = (img, code)
            d.src, d.dst, d.dtype = w.data_ptr(), img.data_ptr(), code
            d.ntaps, d.K, d.N, d.sk, d.sn, d.st = Kw, K, N, sk, sn, 1
            d.scale = img.data_ptr() + Kw * K * N if code == L.FP8 else None
            self.fp8 = getattr(self, "fp8", False) or code == L.FP8
        raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
        self.table = raw.to(dev)
        self.n = len(items)
        self.key = tuple(w.data_ptr() for _, w, _, _ in items)

    def refresh(self):
        if getattr(self, "fp8", False):     # per-tensor scales of the e4m3 images first
            L.check(L.load().sa_pack_scales_multi(_f(self.table), self.n, L.stream()), "sa_pack_scales_multi")
        L.check(L.load().sa_pack_weights_multi(_f(self.table), self.n, 64, L.stream()),
                "sa_pack_weights_multi")


@functools.lru_cache(maxsize=None)
def _conv_geometry(cin, cout, u, Lout):
    """tiles per utterance of a launch = slabs of its stats / pro_stats / colsum outputs (cached: the
    tile policy is fixed per process; conv_impl() clears the cache when its tile-row knob changes it)"""
    return L.load().sa_conv_gemm_ntiles(cin, cout, u, Lout)


def conv_impl(pingpong=False, tile_rows=0, ws=True):
    """kernel choice (A/B timing, kernel tests).  Default: the weight-stationary kernels (sa_conv_ws.hip,
    sa_conv_wsd.hip) for the large bf16x3 launches they cover, the one-tile-per-workgroup kernel for
    everything else; ws=False: one-tile kernel only.  tile_rows: tile height of the one-tile kernel
    (0 = policy).  pingpong is accepted only so that a caller asking for the removed kernel is told so."""
    if pingpong:
        raise L.SaHipError("the ping-pong conv kernel was removed (it tied the one-tile kernel forward and lost "
                           "on the fused data gradients: DESIGN.md section 4); use ws=True or ws=False")
    lib = L.load()
    L.check(lib.sa_conv_gemm_set_impl(2 if ws else 0), "sa_conv_gemm_set_impl")
    L.check(lib.sa_conv_gemm_set_tile_rows(int(tile_rows)), "sa_conv_gemm_set_tile_rows")
    _conv_geometry.cache_clear()


def conv_gemm(x, wp, bias, cin, cout, sa, u, phases, Lout, s1=None, t1=None, s2=None, t2=None,
              swish=False, relu=False, want_stats=False, out=None, code=None, ep=None, a_out=None,
              nb=None, want_pro_stats=False):
    """x [B, Lin, cin] -> y [B, Lout, cout] (+ per-tile partial stats [B, ntiles, cout, 2]).
    ep: fused backward epilogue dict(mode=1|2, x=, g2=, s1=, t1=, mean=, rstd=, xp_is_act=,
    per_c=) -- see SaConvArgs.ep_* in include/sa_hip.h.  a_out: optional bf16 [B, Lin, cin] tensor
    that receives the transformed input rows (the A operand of wgrad(..., x_pre=True)).
    nb=dict(x=, c1=, c2=, c3=, per_c=, relu_mask=, want_colsum=): normalisation-backward prologue
    (SaConvArgs.nb_*); with want_colsum the per-tile column sums [B, ntiles, cin] are returned last.
    want_pro_stats: also return per-tile (sum, sumsq) of the transformed input rows [B, ntiles, cin, 2]."""
    lib = L.load()
    B, Lin, _ = x.shape
    assert x.shape[2] == cin
    y = out if out is not None else torch.empty(B, Lout, cout, dtype=x.dtype, device=x.device)
    kc = L.dt_code(x.dtype) if code is None else code
    nt = _conv_geometry(cin, cout, u, Lout)
    stats = torch.empty(B, nt, cout, 2, dtype=torch.float32, device=x.device) if want_stats else None
    a = L.SaConvArgs()
    a.x, a.wp, a.bias, a.y = _f(x), _f(wp), _f(bias), _f(y)
    a.s1, a.t1, a.s2, a.t2 = _f(s1), _f(t1), _f(s2), _f(t2)
    a.swish, a.relu, a.stats = int(swish), int(relu), _f(stats)
    a.B, a.Lin, a.Lout = B, Lin, Lout
    a.taps = L.make_taps(phases)
    if kc == L.FP8:                          # the scale sits behind the e4m3 image
        a.wscale = C.c_void_p(wp.data_ptr() + wp.numel() - 4)
    if a_out is not None:
        assert a_out.dtype == torch.bfloat16 and a_out.shape == x.shape
        a.a_out = _f(a_out)
    pro_stats = None
    if want_pro_stats:
        pro_stats = torch.empty(B, nt, cin, 2, dtype=torch.float32, device=x.device)
        a.pro_stats = _f(pro_stats)
    colsum = None
    if nb:
        assert nb["x"].shape == x.shape and nb["x"].dtype == x.dtype
        a.nb_x, a.nb_c1, a.nb_c2, a.nb_c3 = _f(nb["x"]), _f(nb["c1"]), _f(nb["c2"]), _f(nb["c3"])
        a.nb_bstride, a.nb_relu_mask = (0 if nb.get("per_c") else cin), int(bool(nb.get("relu_mask")))
        if nb.get("want_colsum"):
            colsum = torch.empty(B, nt, cin, dtype=torch.float32, device=x.device)
            a.nb_colsum = _f(colsum)
    if ep:
        a.ep_mode, a.ep_xp_is_act = int(ep["mode"]), int(bool(ep.get("xp_is_act")))
        a.ep_bstride = 0 if ep.get("per_c") else cout
        a.ep_x, a.ep_g2 = _f(ep["x"]), _f(ep.get("g2"))
        a.ep_s1, a.ep_t1 = _f(ep.get("s1")), _f(ep.get("t1"))
        a.ep_mean, a.ep_rstd = _f(ep.get("mean")), _f(ep.get("rstd"))
        if ep.get("g2k") is not None:
            a.ep_g2k1, a.ep_g2k2, a.ep_g2k3 = (_f(t) for t in ep["g2k"])
    e0 = PROFILE.start(f"conv_gemm({cin},{cout},{sa},{u})") if PROFILE.key else None
    L.check(lib.sa_conv_gemm(kc, cin, cout, sa, u, C.byref(a), L.stream()),
            f"sa_conv_gemm({cin},{cout},{sa},{u})")
    if e0 is not None:
        ntap = sum(len(p) for p in phases)
        esz = x.element_size()
        extra = (a_out.numel() * 2 if a_out is not None else 0)        # bf16 operand cache written
        if ep:
            extra += y.numel() * esz * (2 if ep.get("g2") is not None else 1)   # stored forward tensor (+ 2nd gradient) read
        if nb:
            extra += x.numel() * esz                                             # stored forward tensor of the layer above
        io = (x.numel() + y.numel()) * esz
        route = lib.sa_conv_gemm_route(kc, cin, cout, sa, u, C.byref(a))
        tname = {L.F32: "float", L.BF16: "bf16_t", L.BF16X3: "bf16x3_t", L.BF16X1F: "bf16x1f_t", L.FP8: "fp8_t"}[kc]
        ws_mode = (5 if s2 is not None else 0) if s1 is None else 3 if want_pro_stats else 4 if s2 is not None else 1
        # (the five instances <taps, span, prologue, epilogue> of the fused data-gradient kernel are ONE
        # kernel for the roofline record: same source, same structure, 1 launch per step each)
        kind = (f"sa_conv_wsd_kernel ({tname}, {cin}->{cout}; 5 instances)" if route == 3 else
                f"sa_conv_ws_kernel<{ws_mode},{ntap}> ({tname}, {cin}->{cout})" if route == 2 else
                f"sa_conv_gemm_kernel<{tname},{cin},{cout},{sa},{u}{',nb prologue' if nb else ''}>")
        PROFILE.stop(e0, io + ntap * cin * cout * esz + extra,
                     2 * B * (-(-Lout // u)) * ntap * cin * cout,
                     alg_bytes=io + (y.numel() * esz if ep else 0), kind=kind)
    out_t = (y, stats) if want_stats else (y,)
    if nb and nb.get("want_colsum"):
        out_t = out_t + (colsum,)
    if want_pro_stats:
        out_t = out_t + (pro_stats,)
    return out_t if len(out_t) > 1 else y


WGRAD_TARGET_WGS = {True: 256, False: 512}


def wgrad(x, dy, cin, cout, sa, u, taps, Mrows, dst, dst_strides, s1=None, t1=None, s2=None,
          t2=None, swish=False, accumulate=False, target_wgs=None, code=None, x_pre=False,
          dy_pre=False, defer=None):
    """taps: list of (row_offset, phase) per weight tap.  dst: fp32 parameter-gradient tensor in
    PyTorch layout; dst_strides = (s_ci, s_co, s_tap).  x_pre: x is the bf16 a_out tensor of the
    forward conv_gemm (already transformed; s1..swish are ignored); dy_pre: dy is the bf16 a_out of
    the data-gradient conv_gemm that formed it in its normalisation-backward prologue."""
    lib = L.load()
    B, Lin, _ = x.shape
    Ldy = dy.shape[1]
    if x_pre:
        assert x.dtype == torch.bfloat16 and code in (L.BF16X1F, L.BF16)
    nt = len(taps)
    kw = lib.sa_wgrad_kw(cin, cout)
    if target_wgs is None:
        # one 8-wave workgroup (128-wide channel blocks) or two-three 4-wave ones fit a CU: size
        # the row chunks so that the grid is one resident wave of workgroups over the 256 CUs
        target_wgs = WGRAD_TARGET_WGS[(cin // 32) * (cout // 32) >= 8]
    chunk = max(64, -(-Mrows * B // target_wgs))
    chunk = -(-chunk // 64) * 64
    nchunk = -(-Mrows // chunk)
    slabs = torch.empty(B * nchunk * kw * nt * cin * cout, dtype=torch.float32, device=x.device)
    a = L.SaWgradArgs()
    a.x, a.dy, a.slabs = _f(x), _f(dy), _f(slabs)
    a.s1, a.t1, a.s2, a.t2, a.swish = _f(s1), _f(t1), _f(s2), _f(t2), int(swish)
    a.B, a.Lin, a.Ldy, a.Mrows, a.chunk, a.nchunk, a.ntaps = B, Lin, Ldy, Mrows, chunk, nchunk, nt
    for i, (off, ph) in enumerate(taps):
        a.off[i], a.ph[i] = off, ph
    a.x_pre, a.dy_pre = int(x_pre), int(dy_pre)
    if dy_pre:
        assert x_pre and dy.dtype == torch.bfloat16
    L.check(lib.sa_wgrad((L.BF16X1F if dy_pre else L.dt_code(dy.dtype)) if code is None else code, cin, cout, sa, u,
                         C.byref(a), L.stream()),
            f"sa_wgrad({cin},{cout},{sa},{u})")
    sk, sn, st = dst_strides
    if defer is not None:           # the reducer joins the others of its backward stage (wgrad_reduce_multi)
        defer.append((slabs, dst, B * nchunk * kw, nt, cin, cout, sk, sn, st, int(accumulate)))
        return dst
    L.check(lib.sa_wgrad_reduce(_f(slabs), _f(dst), B * nchunk * kw, nt, cin, cout, sk, sn, st,
                                int(accumulate), L.stream()), "sa_wgrad_reduce")
    return dst


def wgrad_reduce_multi(items):
    """items: the deferred reducers of wgrad(..., defer=items): (slabs, dst, nslab, ntaps, cin, cout, sk, sn, st,
    accumulate) each -- one launch per eight of them (sa_wgrad_reduce_multi; same bits as one launch each)"""
    lib = L.load()
    for i0 in range(0, len(items), L.WRED_MAX):
        m = L.SaWredMulti()
        chunk = items[i0:i0 + L.WRED_MAX]
        m.n = len(chunk)
        for d, (slabs, dst, nslab, nt, cin, cout, sk, sn, st, acc) in zip(m.d, chunk):
            d.slabs, d.dst = slabs.data_ptr(), dst.data_ptr()
            d.nslab, d.ntaps, d.cin, d.cout, d.sk, d.sn, d.st, d.accumulate = nslab, nt, cin, cout, sk, sn, st, acc
        L.check(lib.sa_wgrad_reduce_multi(C.byref(m), L.stream()), "sa_wgrad_reduce_multi")


def conv1toC(x, w, bias, dtype, flip=False, want_stats=False, ep=None):
    """ep=dict(x=, s1=, t1=, mean=, rstd=): fused [InstanceNorm -> x*sigmoid(x)] backward epilogue."""
    lib = L.load()
    B, Ln = x.shape
    y = torch.empty(B, Ln, 32, dtype=dtype, device=x.device)
    nt = lib.sa_conv1toC_ntiles(Ln)
    stats = torch.empty(B, nt, 32, 2, dtype=torch.float32, device=x.device) if want_stats else None
    e = ep or {}
    L.check(lib.sa_conv1toC(L.dt_code(dtype), _f(x), _f(w), _f(bias), _f(y), B, Ln, int(flip),
                            _f(stats), _f(e.get("x")), _f(e.get("s1")), _f(e.get("t1")),
                            _f(e.get("mean")), _f(e.get("rstd")), L.stream()), "sa_conv1toC")
    return (y, stats) if want_stats else y


def convCto1(x, w, bias, s1=None, t1=None, swish=False, flip=False):
    lib = L.load()
    B, Ln, _ = x.shape
    y = torch.empty(B, Ln, dtype=torch.float32, device=x.device)
    L.check(lib.sa_convCto1(L.dt_code(x.dtype), _f(x), _f(w), _f(bias), _f(y), B, Ln, _f(s1), _f(t1),
                            int(swish), int(flip), L.stream()), "sa_convCto1")
    return y


def wgrad1C(u, v, dst, flip=False, s1=None, t1=None, swish=False, accumulate=False, chunk=2048):
    lib = L.load()
    B, Ln = u.shape
    nch = lib.sa_wgrad1C_nchunk(Ln, chunk)
    slabs = torch.empty(B * nch, 32 * 15, dtype=torch.float32, device=u.device)
    L.check(lib.sa_wgrad1C(L.dt_code(v.dtype), _f(u), _f(v), _f(slabs), B, Ln, chunk, int(flip),
                           _f(s1), _f(t1), int(swish), L.stream()), "sa_wgrad1C")
    L.check(lib.sa_sum_slabs(_f(slabs), _f(dst), B * nch, 32 * 15, int(accumulate), L.stream()),
            "sa_sum_slabs")
    return dst


def bwd1C(u, v, w, dst, s1, t1, mean, rstd, flip=True, accumulate=False, chunk=2048):
    """backward of the 32 -> 1 layer in one launch and one read of v: (g, stats, dst) with the bits of
    conv1toC(u, w, None, v.dtype, flip, want_stats=True, ep=dict(x=v, s1=, t1=, mean=, rstd=)) and of
    wgrad1C(u, v, dst, flip, s1, t1, swish=True, accumulate=, chunk=)"""
    lib = L.load()
    B, Ln = u.shape
    nch = lib.sa_wgrad1C_nchunk(Ln, chunk)
    g = torch.empty(B, Ln, 32, dtype=v.dtype, device=u.device)
    stats = torch.empty(B, lib.sa_conv1toC_ntiles(Ln), 32, 2, dtype=torch.float32, device=u.device)
    slabs = torch.empty(B * nch, 32 * 15, dtype=torch.float32, device=u.device)
    L.check(lib.sa_bwd1C(L.dt_code(v.dtype), _f(u), _f(v), _f(w), _f(g), _f(stats), _f(slabs), B, Ln, chunk,
                         int(flip), _f(s1), _f(t1), _f(mean), _f(rstd), L.stream()), "sa_bwd1C")
    L.check(lib.sa_sum_slabs(_f(slabs), _f(dst), B * nch, 32 * 15, int(accumulate), L.stream()),
            "sa_sum_slabs")
    return g, stats, dst


def sum_partials(part, nbatch, n=None, rows=False):
    """part [nbatch][nslab][n] (contiguous) -> [nbatch, n] fixed-order sums.  n defaults to the
    product of the last two dims (the [.., C, 2] layout of the statistics slabs).  rows=True (with
    nbatch == 1): return the per-utterance partial rows [R, n] of the two-level reduction instead of
    their sum -- the BatchNorm finalisers add them (fin_bn_fwd / fin_norm_bwd take R rows)."""
    lib = L.load()
    if n is None:
        n = part.shape[-2] * part.shape[-1]
    total = part.numel()
    nslab = total // (nbatch * n)
    if nbatch == 1 and nslab >= 512 and part.dim() == 4 and part.shape[0] > 1:
        # two levels (per utterance, then over utterances): keeps the first level wide
        R = part.shape[0]
        mid = torch.empty(R, n, dtype=torch.float64, device=part.device)
        L.check(lib.sa_sum_partials(_f(part), _f(mid), R, nslab // R, n, L.stream()), "sa_sum_partials")
        if rows:
            return mid
        out = torch.empty(1, n, dtype=torch.float64, device=part.device)
        L.check(lib.sa_sum_rows_d(_f(mid), _f(out), R, n, L.stream()), "sa_sum_rows_d")
        return out
    out = torch.empty(nbatch, n, dtype=torch.float64, device=part.device)
    L.check(lib.sa_sum_partials(_f(part), _f(out), nbatch, nslab, n, L.stream()), "sa_sum_partials")
    return out


def fin_in_fwd(sums, B, Cc, n, gamma, beta, eps=1e-5):
    lib = L.load()
    o = torch.empty(4, B, Cc, dtype=torch.float32, device=sums.device)
    L.check(lib.sa_fin_in_fwd(_f(sums), B, Cc, n, _f(gamma), _f(beta), C.c_float(eps), _f(o[0]),
                              _f(o[1]), _f(o[2]), _f(o[3]), L.stream()), "sa_fin_in_fwd")
    return o[0], o[1], o[2], o[3]          # mean, rstd, scale, shift


def fin_bn_fwd(sums, Cc, count, gamma, beta, run_mean=None, run_var=None, eps=1e-5, momentum=0.1,
               count_dev=None):
    """count_dev: fp64 device scalar holding the (all-reduced) element count; overrides count."""
    lib = L.load()
    o = torch.empty(4, Cc, dtype=torch.float32, device=sums.device)
    L.check(lib.sa_fin_bn_fwd(_f(sums), sums.numel() // (2 * Cc), Cc, C.c_double(count), _f(gamma), _f(beta), C.c_float(eps),
                              C.c_float(momentum), _f(run_mean), _f(run_var), _f(o[0]), _f(o[1]),
                              _f(o[2]), _f(o[3]), _f(count_dev), L.stream()), "sa_fin_bn_fwd")
    return o[0], o[1], o[2], o[3]


def fin_bn_eval(Cc, gamma, beta, run_mean, run_var, eps=1e-5):
    lib = L.load()
    o = torch.empty(4, Cc, dtype=torch.float32, device=gamma.device)
    L.check(lib.sa_fin_bn_eval(Cc, _f(gamma), _f(beta), C.c_float(eps), _f(run_mean), _f(run_var),
                               _f(o[0]), _f(o[1]), _f(o[2]), _f(o[3]), L.stream()), "sa_fin_bn_eval")
    return o[0], o[1], o[2], o[3]


def fin_norm_bwd(sums, lsums, groups, Cc, n, gamma, mean, rstd, sign=1.0, dgamma=None, dbeta=None,
                 n_dev=None):
    lib = L.load()
    o = torch.empty(3, groups, dtype=torch.float32, device=sums.device)
    R = sums.numel() // (2 * groups)
    assert lsums is None or lsums.numel() == sums.numel()
    L.check(lib.sa_fin_norm_bwd(_f(sums), _f(lsums), R, groups, Cc, C.c_double(n), _f(gamma), _f(mean),
                                _f(rstd), C.c_float(sign), _f(o[0]), _f(o[1]), _f(o[2]), _f(dgamma),
                                _f(dbeta), _f(n_dev), L.stream()), "sa_fin_norm_bwd")
    return o[0], o[1], o[2]


def bias_multi(items):
    """items: [(part [nbatch, nslab, C(, ncomp)] fp32 slabs, nbatch, C, ncomp, db fp32 [C])]: the bias gradients
    of several layers in two launches (sa_bias_multi; same bits as sum_partials + fin_bias per layer)."""
    lib = L.load()
    dev = items[0][0].device
    rows = torch.empty(sum(nb * cc for _, nb, cc, _, _ in items), dtype=torch.float64, device=dev)
    rp, esz = rows.data_ptr(), 8
    for i0 in range(0, len(items), L.BIAS_MAX):
        m = L.SaBiasMulti()
        chunk = items[i0:i0 + L.BIAS_MAX]
        m.n = len(chunk)
        for d, (part, nb, cc, ncomp, db) in zip(m.d, chunk):
            d.part, d.rows, d.db = part.data_ptr(), rp, db.data_ptr()
            d.nbatch, d.nslab, d.C, d.ncomp = nb, part.numel() // (nb * cc * ncomp), cc, ncomp
            rp += nb * cc * esz
        L.check(lib.sa_bias_multi(C.byref(m), L.stream()), "sa_bias_multi")


def fin_bias(sums, B, Cc, db, ncomp=2):
    """db[c] = sum_b sums[b][c][0]; sums [B, Cc, ncomp] fp64."""
    L.check(L.load().sa_fin_bias(_f(sums), B, Cc, ncomp, _f(db), L.stream()), "sa_fin_bias")
    return db


def ew(kind, g, x, Cc, out=None, g2=None, s1=None, t1=None, mean=None, rstd=None, c1=None, c2=None,
       c3=None, actbwd=False, xp_is_act=False, relu_mask=False, per_c=False, want_stats=True):
    """kind: "stats" | "apply".  Returns partial stats [B, ntiles, C, 2] (or None)."""
    lib = L.load()
    B, Ln, _ = x.shape
    nt = lib.sa_ew_ntiles(Ln)
    stats = torch.empty(B, nt, Cc, 2, dtype=torch.float32, device=x.device) if want_stats else None
    a = L.SaEwArgs()
    a.g, a.g2, a.x, a.out = _f(g), _f(g2), _f(x), _f(out)
    a.s1, a.t1, a.mean, a.rstd = _f(s1), _f(t1), _f(mean), _f(rstd)
    a.c1, a.c2, a.c3 = _f(c1), _f(c2), _f(c3)
    a.actbwd, a.xp_is_act, a.relu_mask = int(actbwd), int(xp_is_act), int(relu_mask)
    a.bstride = 0 if per_c else Cc
    a.stats, a.B, a.L = _f(stats), B, Ln
    fn = lib.sa_ew_stats if kind == "stats" else lib.sa_ew_apply
    L.check(fn(L.dt_code(x.dtype), Cc, C.byref(a), L.stream()), f"sa_ew_{kind}")
    return stats


def pooling_noise(setting, B, Cc, device):
    """speechbrain's StatisticsPooling adds eps*U[1,9] to the pooled mean on every call: the [B, Cc] draw
    in [0, 1] behind it (_get_gauss_noise).  None / False: no noise; a tensor fixes the draw; True draws."""
    if setting is None or setting is False:
        return None
    if torch.is_tensor(setting):
        return setting.to(device=device, dtype=torch.float32).contiguous()
    g = torch.randn(B, Cc, device=device)
    g = g - g.min()
    return (g / g.max()).contiguous()


def pooling_noise_raw(setting, B, Cc, device):
    """pooling_noise for pool_fwd(fused=True): (noise, raw).  True draws the same torch.randn and hands it over
    as it is (raw = True: sa_pool_gather_fin normalises it, the bits of pooling_noise's three ATen steps)."""
    if setting is True:
        return torch.randn(B, Cc, device=device), True
    return pooling_noise(setting, B, Cc, device), False


def pool_fwd(r, scale, shift, noise=None, eps=1e-5, fused=False, raw=False):
    """fused: sa_pool_gather_fin instead of sa_pool_gather + sa_pool_fin (same bits); raw (fused only): noise is
    the N(0,1) draw, normalised to [0, 1] in that launch"""
    lib = L.load()
    B, Ln, _ = r.shape
    nseg = lib.sa_pool_nseg(B)
    part = torch.empty(B, nseg, 128, 128, 2, dtype=torch.float32, device=r.device)
    L.check(lib.sa_pool_fwd(L.dt_code(r.dtype), _f(r), _f(scale), _f(shift), _f(part), B, Ln, nseg,
                            L.stream()), "sa_pool_fwd")
    pooled = torch.empty(B, 256, dtype=torch.float32, device=r.device)
    mean = torch.empty(B, 128, dtype=torch.float32, device=r.device)
    sd = torch.empty(B, 128, dtype=torch.float32, device=r.device)
    if fused:
        if noise is not None and (noise.numel() != B * 128 or noise.dtype != torch.float32):
            raise L.SaHipError(f"pooling noise must be fp32 [{B}, 128], got {noise.dtype} {tuple(noise.shape)}")
        L.check(lib.sa_pool_gather_fin(_f(part), B, nseg, Ln, _f(noise), int(bool(raw)), C.c_float(eps), _f(pooled),
                                       _f(mean), _f(sd), L.stream()), "sa_pool_gather_fin")
        return pooled, mean, sd
    if raw:
        raise L.SaHipError("raw pooling noise needs fused=True")
    sums = torch.empty(B, 128, 2, dtype=torch.float64, device=r.device)
    L.check(lib.sa_pool_gather(_f(part), B, nseg, Ln, _f(sums), L.stream()), "sa_pool_gather")
    L.check(lib.sa_pool_fin(_f(sums), B, Ln, _f(noise), C.c_float(eps), _f(pooled), _f(mean), _f(sd),
                            L.stream()), "sa_pool_fin")
    return pooled, mean, sd


def pool_bwd(r, scale, shift, dpooled, mean, sd, bn=None):
    """bn=(mean[128], rstd[128]) of the BatchNorm that produced the pooled tensor: also return the
    partial (sum g, sum g*xhat) slabs [B, ntiles, 128, 2] of its backward."""
    lib = L.load()
    B, Ln, _ = r.shape
    g = torch.empty_like(r)
    st = torch.empty(B, -(-Ln // 256), 128, 2, dtype=torch.float32, device=r.device) if bn else None
    L.check(lib.sa_pool_bwd(L.dt_code(r.dtype), _f(r), _f(scale), _f(shift), _f(dpooled), _f(mean),
                            _f(sd), _f(g), B, Ln, _f(bn[0]) if bn else None, _f(bn[1]) if bn else None,
                            _f(st), L.stream()), "sa_pool_bwd")
    return (g, st) if bn else g


def dense(X, W, bias, N, K, ps=None, pt=None, relu=False, transpose_w=False):
    """Y[M,N] = act(P(X)[M,K] @ Wm + bias).  W is an nn.Linear weight; transpose_w=False uses
    Wm[k][n] = W[n][k] (forward), True uses Wm[k][n] = W[k][n] (data gradient)."""
    lib = L.load()
    M = X.shape[0]
    Y = torch.empty(M, N, dtype=torch.float32, device=X.device)
    sbk, sbn = (W.shape[1], 1) if transpose_w else (1, W.shape[1])
    L.check(lib.sa_dense(_f(X), X.shape[1], _f(ps), _f(pt), _f(W), sbk, sbn, _f(bias), _f(Y), N, M, N,
                         K, int(relu), L.stream()), "sa_dense")
    return Y


def colsums(X, H=None, hmean=None, hrstd=None, out0=None, out1=None):
    """out0 / out1: fp32 [N] tensors (parameter-gradient views) that receive columns 0 / 1 of the
    fp64 sums rounded to fp32 -- no separate copy launch"""
    lib = L.load()
    M, N = X.shape
    s = torch.empty(N, 2, dtype=torch.float64, device=X.device)
    for o in (out0, out1):
        assert o is None or (o.dtype == torch.float32 and o.numel() == N and o.is_contiguous())
    L.check(lib.sa_colsums(_f(X), _f(H), _f(hmean), _f(hrstd), M, N, _f(s), _f(out0), _f(out1), L.stream()),
            "sa_colsums")
    return s


def bn2d_bwd(G, H, sums, count, gamma, mean, rstd, relu_mask, count_dev=None):
    lib = L.load()
    M, N = G.shape
    dH = torch.empty_like(G)
    L.check(lib.sa_bn2d_bwd(_f(G), _f(H), _f(sums), C.c_double(count), _f(gamma), _f(mean), _f(rstd),
                            int(relu_mask), M, N, _f(dH), _f(count_dev), L.stream()), "sa_bn2d_bwd")
    return dH


def dense_wgrad(dY, X, dW, ps=None, pt=None):
    lib = L.load()
    M, N = dY.shape
    K = X.shape[1]
    L.check(lib.sa_dense_wgrad(_f(dY), _f(X), _f(ps), _f(pt), M, N, K, _f(dW), L.stream()),
            "sa_dense_wgrad")
    return dW


def head_max_rows():
    return L.load().sa_head_max_rows()


def head_fwd(pooled, P, bn1, bn2, eps=1e-5, momentum=0.1):
    """The whole FC head in one launch (sa_head_fwd).  P: the sex_classifier.classify.* parameters by
    short name ("0.weight" ...); bn1 / bn2: the BatchNorm modules (running statistics are updated).
    Returns H1, f1 (mean, rstd, scale, shift), H2, f2, logp."""
    M = pooled.shape[0]
    dev = pooled.device
    H1 = torch.empty(M, 128, dtype=torch.float32, device=dev)
    H2 = torch.empty(M, 64, dtype=torch.float32, device=dev)
    f1 = torch.empty(4, 128, dtype=torch.float32, device=dev)
    f2 = torch.empty(4, 64, dtype=torch.float32, device=dev)
    logp = torch.empty(M, 2, dtype=torch.float32, device=dev)
    L.check(L.load().sa_head_fwd(_f(pooled), _f(P["0.weight"]), _f(P["0.bias"]), _f(P["2.weight"]), _f(P["2.bias"]),
                                 _f(bn1.running_mean), _f(bn1.running_var), _f(P["3.weight"]), _f(P["3.bias"]),
                                 _f(P["5.weight"]), _f(P["5.bias"]), _f(bn2.running_mean), _f(bn2.running_var),
                                 _f(P["6.weight"]), _f(P["6.bias"]), _f(H1), _f(f1), _f(H2), _f(f2), _f(logp), M,
                                 C.c_float(eps), C.c_float(momentum), L.stream()), "sa_head_fwd")
    return H1, tuple(f1[i] for i in range(4)), H2, tuple(f2[i] for i in range(4)), logp


def head_bwd(dlogp, logp, pooled, H1, f1, H2, f2, P, grads, wide=False):
    """sa_head_bwd: grads maps the short parameter names to fp32 gradient views (or None); returns dpooled.
    f1 / f2: the tuples head_fwd returned (rows of one [4][N] tensor).  wide: sa_head_bwd_wide, the same
    backward (same bits) over 16 workgroups."""
    M = pooled.shape[0]
    dpooled = torch.empty(M, 256, dtype=torch.float32, device=pooled.device)
    g = lambda k: _f(grads.get(k))
    lib = L.load()
    entry, name = (lib.sa_head_bwd_wide, "sa_head_bwd_wide") if wide else (lib.sa_head_bwd, "sa_head_bwd")
    L.check(entry(_f(dlogp), _f(logp), _f(pooled), _f(H1), _f(f1[0]), _f(H2), _f(f2[0]),
                  _f(P["0.weight"]), _f(P["2.weight"]), _f(P["3.weight"]), _f(P["5.weight"]),
                  _f(P["6.weight"]), g("0.weight"), g("0.bias"), g("2.weight"), g("2.bias"),
                  g("3.weight"), g("3.bias"), g("5.weight"), g("5.bias"), g("6.weight"), g("6.bias"),
                  _f(dpooled), M, L.stream()), name)
    return dpooled


def log_softmax(X):
    Y = torch.empty_like(X)
    L.check(L.load().sa_log_softmax(_f(X), _f(Y), X.shape[0], X.shape[1], L.stream()), "sa_log_softmax")
    return Y


def log_softmax_bwd(dY, Y):
    dX = torch.empty_like(Y)
    L.check(L.load().sa_log_softmax_bwd(_f(dY), _f(Y), _f(dX), Y.shape[0], Y.shape[1], L.stream()),
            "sa_log_softmax_bwd")
    return dX


def recon_loss(a, b, kind, want_grad=True):
    """kind "l1" | "mse"; returns (loss[1], grad like a or None)."""
    lib = L.load()
    n = a.numel()
    # the kernel reads float4: a contiguous view at a storage offset that is not a multiple of four
    # elements (x.reshape(-1)[1:]) is copied to a fresh, aligned allocation (never in the train step)
    if a.data_ptr() % 16:
        a = a.clone()
    if b.data_ptr() % 16:
        b = b.clone()
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    grad = torch.empty_like(a) if want_grad else None
    ws = torch.empty(lib.sa_loss_workspace_bytes() // 8, dtype=torch.float64, device=a.device)
    L.check(lib.sa_recon_loss(_f(a), _f(b), C.c_longlong(n), 0 if kind == "l1" else 1, _f(grad),
                              _f(loss), _f(ws), L.stream()), "sa_recon_loss")
    return loss, grad


def cls_losses(logp, label, want_grad=True):
    lib = L.load()
    B, NC = logp.shape
    out = torch.empty(2, dtype=torch.float32, device=logp.device)
    dn = torch.empty_like(logp) if want_grad else None
    dc = torch.empty_like(logp) if want_grad else None
    L.check(lib.sa_cls_losses(_f(logp), _f(label), B, NC, _f(out), _f(dn), _f(dc), L.stream()),
            "sa_cls_losses")
    return out, dn, dc


def step_loss(pred, target, kind, logp, label, w_recon, w_sex, nonfinite=None):
    """The loss tail of the ConvAE train step in two launches (sa_recon_loss_part + sa_step_loss) instead of
    recon_loss + cls_losses + the weighted sum, its autograd graph and the non-finite count on ATen kernels.
    pred / target: contiguous fp32 of one shape; logp [B, NC]; label int64 [B]; nonfinite: the device int32
    counter that receives `+= !isfinite(total)` (or None).  Returns out = (recon, sex, total) and the gradients
    the scalar graph would hand to pred and logp, bit for bit: d_pred = g * fl(1.0f * w_recon) with g the
    gradient recon_loss returns, d_logp = dnll * fl(1.0f * w_sex)."""
    lib = L.load()
    n = pred.numel()
    if pred.data_ptr() % 16:
        pred = pred.clone()
    if target.data_ptr() % 16:
        target = target.clone()
    B, NC = logp.shape
    dev = pred.device
    ws = torch.empty(lib.sa_loss_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    d_pred = torch.empty_like(pred)
    d_logp = torch.empty_like(logp)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    # (c_float rounds the Python float to fp32 as torch rounds a scalar operand; 1.0f * weight is exact)
    L.check(lib.sa_recon_loss_part(_f(pred), _f(target), C.c_longlong(n), 0 if kind == "l1" else 1, _f(d_pred),
                                   C.c_float(w_recon), _f(ws), L.stream()), "sa_recon_loss_part")
    L.check(lib.sa_step_loss(_f(ws), C.c_longlong(n), _f(logp), _f(label), B, NC, C.c_float(w_recon),
                             C.c_float(w_sex), _f(out), _f(d_logp), _f(nonfinite), L.stream()), "sa_step_loss")
    return out, d_pred, d_logp


def cosine_loss(x1, x2, want_grad=False):
    lib = L.load()
    B, S, D = x1.shape
    rl = torch.empty(B * S, dtype=torch.float32, device=x1.device)
    loss = torch.empty(1, dtype=torch.float32, device=x1.device)
    dx1 = torch.empty_like(x1) if want_grad else None
    L.check(lib.sa_cosine_loss(_f(x1), _f(x2), B, S, D, _f(rl), _f(loss), _f(dx1), L.stream()),
            "sa_cosine_loss")
    return loss, dx1


def cosine_rows(x1, x2):
    """per-row cosine similarity of two [B, D] tensors (sa_cosine_loss's row output: 1 - loss of
    the row; eps 1e-6 on |x1||x2|, where torch.nn.CosineSimilarity(eps=1e-8) of the reference's
    evaluation hook differs only for vectors of norm < 1e-3)."""
    lib = L.load()
    B, D = x1.shape
    x1, x2 = x1.contiguous().float(), x2.contiguous().float()
    rl = torch.empty(B, dtype=torch.float32, device=x1.device)
    loss = torch.empty(1, dtype=torch.float32, device=x1.device)
    L.check(lib.sa_cosine_loss(_f(x1), _f(x2), B, 1, D, _f(rl), _f(loss), None, L.stream()),
            "sa_cosine_loss")
    return 1.0 - rl


def cluster_mi(X, y, idx=None, ncls=2, k=3):
    lib = L.load()
    iters, n = (idx.shape if idx is not None else (1, X.shape[0]))
    mi = torch.empty(iters, dtype=torch.float32, device=X.device)
    L.check(lib.sa_cluster_mi(_f(X), _f(y), _f(idx), iters, n, X.shape[1], ncls, k, _f(mi), L.stream()),
            "sa_cluster_mi")
    return mi


# ---- element-wise passes of the frozen recogniser (csrc/sa_asr.hip; asr.py) ----
def add_layernorm(x, r, gamma, beta, eps, save):
    """y = LayerNorm(bf16(x + r)) * gamma + beta over the last dimension (r may be None); bf16 tensors.
    save: also return the stored sum s and the statistics the backward re-reads."""
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    s = torch.empty_like(x) if save else None
    stat = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if save else None
    L.check(L.load().sa_add_layernorm_fwd(_f(x), _f(r), _f(gamma), _f(beta), _f(y), _f(s), _f(stat), rows, d,
                                          C.c_float(eps), L.stream()), "sa_add_layernorm_fwd")
    return y, s, stat


def layernorm_bwd(dy, s, stat, gamma):
    d = s.shape[-1]
    ds = torch.empty_like(s)
    L.check(L.load().sa_layernorm_bwd(_f(dy), _f(s), _f(stat), _f(gamma), _f(ds), s.numel() // d, d, L.stream()),
            "sa_layernorm_bwd")
    return ds


def reflect_pad(x):
    """[B, T, F, C] bf16 -> [B, T + 2, F + 2, C], reflect padding of T and F by one"""
    B, T, F_, Cc = x.shape
    y = torch.empty(B, T + 2, F_ + 2, Cc, dtype=x.dtype, device=x.device)
    L.check(L.load().sa_reflect_pad_fwd(_f(x), _f(y), B, T, F_, Cc, L.stream()), "sa_reflect_pad_fwd")
    return y


def reflect_pad_bwd(dy):
    B, T2, F2, Cc = dy.shape
    dx = torch.empty(B, T2 - 2, F2 - 2, Cc, dtype=dy.dtype, device=dy.device)
    L.check(L.load().sa_reflect_pad_bwd(_f(dy), _f(dx), B, T2 - 2, F2 - 2, Cc, L.stream()), "sa_reflect_pad_bwd")
    return dx


def ln_leaky(x, gamma, beta, eps, slope, save):
    """leaky_relu(LayerNorm over the trailing gamma.numel() elements): [rows, d] bf16, d in {5120, 10240}"""
    d = gamma.numel()
    rows = x.numel() // d
    y = torch.empty_like(x)
    stat = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if save else None
    L.check(L.load().sa_ln_leaky_fwd(_f(x), _f(gamma), _f(beta), _f(y), _f(stat), rows, d, C.c_float(eps),
                                     C.c_float(slope), L.stream()), "sa_ln_leaky_fwd")
    return y, stat


def ln_leaky_bwd(dy, x, stat, gamma, beta, slope):
    d = gamma.numel()
    dx = torch.empty_like(x)
    L.check(L.load().sa_ln_leaky_bwd(_f(dy), _f(x), _f(stat), _f(gamma), _f(beta), _f(dx), x.numel() // d, d,
                                     C.c_float(slope), L.stream()), "sa_ln_leaky_bwd")
    return dx


def asr_block0(x, w, bias, gamma, beta, eps, slope, save):
    """x [B, T, 80] bf16 -> leaky(LayerNorm(conv 1 -> 128, 3 x 3, stride 2, reflect "same")) [B, ceil(T/2), 40, 128]"""
    B, T, F_ = x.shape
    Cc = w.shape[0]
    To = (T - 1) // 2 + 1
    y = torch.empty(B, To, (F_ - 1) // 2 + 1, Cc, dtype=x.dtype, device=x.device)
    stat = torch.empty(B * To, 2, dtype=torch.float32, device=x.device) if save else None
    L.check(L.load().sa_asr_block0_fwd(_f(x), _f(w), _f(bias), _f(gamma), _f(beta), _f(y), _f(stat), B, T, F_, Cc,
                                       C.c_float(eps), C.c_float(slope), L.stream()), "sa_asr_block0_fwd")
    return y, stat


def asr_block0_bwd(dy, x, w, bias, gamma, beta, stat, slope):
    B, T, F_ = x.shape
    To = (T - 1) // 2 + 1
    part = torch.empty(B * To, 3, F_ + 2, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    L.check(L.load().sa_asr_block0_bwd(_f(dy), _f(x), _f(w), _f(bias), _f(gamma), _f(beta), _f(stat), _f(part), _f(dx),
                                       B, T, F_, w.shape[0], C.c_float(slope), L.stream()), "sa_asr_block0_bwd")
    return dx


def clip_flats(flats, max_norm, eps=1e-6):
    """torch.nn.utils.clip_grad_norm_ on flat fp32 gradient buffers, in place (sa_clip_grads); returns the norm"""
    f = L.SaFlats()
    f.n = len(flats)
    for d, t in zip(f.f, flats):
        d.p, d.n = t.data_ptr(), t.numel()
    dev = flats[0].device
    partials = torch.empty(L.FLATS_MAX * 64, dtype=torch.float64, device=dev)
    total = torch.empty((), dtype=torch.float32, device=dev)
    L.check(L.load().sa_clip_grads(C.byref(f), C.c_float(max_norm), C.c_float(eps), _f(partials), _f(total), L.stream()),
            "sa_clip_grads")
    return total


# ---- the arithmetic of torch.optim.Adam(fused=True).step() in one launch (csrc/sa_optim.hip) ----
def _adam_plain(opt):
    """the configuration half of adam_step's conditions: torch.optim.Adam itself, fused, nothing but the plain
    update (no weight decay, amsgrad, maximize, grad scaler, step hooks), scalar betas, lr a host number or the
    capturable optimizer's float32 device scalar"""
    from torch.optim import optimizer as _o
    if type(opt) is not torch.optim.Adam:
        return False
    if getattr(opt, "grad_scale", None) is not None or getattr(opt, "found_inf", None) is not None:
        return False
    if (opt._optimizer_step_pre_hooks or opt._optimizer_step_post_hooks or _o._global_optimizer_pre_hooks
            or _o._global_optimizer_post_hooks):
        return False
    for g in opt.param_groups:
        if (not g.get("fused") or g["weight_decay"] != 0 or g["amsgrad"] or g["maximize"] or g.get("differentiable")
                or g.get("decoupled_weight_decay")):
            return False
        if any(torch.is_tensor(b) for b in g["betas"]) or torch.is_tensor(g["eps"]):
            return False
        lr = g["lr"]
        if torch.is_tensor(lr) and not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1):
            return False
    return True


def _adam_group(opt, group, spans):
    """(key, steps, device) of one param group, or None when a tensor is outside what the kernel covers: every
    parameter with a gradient has state (torch creates it in its first step), everything fp32, contiguous, on one
    GPU.  key: per tensor (param, exp_avg, exp_avg_sq, step pointers, numel, bucket index, element offset in the
    bucket | -1, gradient pointer) -- equal keys mean the cached device table still describes the group"""
    st, key, steps, dev = opt.state, [], [], None
    f32 = torch.float32
    for p in group["params"]:
        g = p.grad
        if g is None:
            continue
        s = st.get(p)
        if not s:
            return None
        step, m, v = s["step"], s["exp_avg"], s["exp_avg_sq"]
        n = p.numel()
        if dev is None:
            dev = p.device
            if dev.type != "cuda":
                return None
        for t in (p, g, m, v):
            if (t.dtype is not f32 or t.device != dev or t.layout is not torch.strided or t.numel() != n
                    or not t.is_contiguous()):
                return None
        if step.dtype is not f32 or step.device != dev or step.numel() != 1 or n == 0:
            return None
        a = g.data_ptr()
        rec = (p.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), n, -1, a)
        for i, (lo, hi) in enumerate(spans):
            if lo <= a and a + 4 * n <= hi:
                rec = rec[:5] + (i, (a - lo) // 4)
                break
        key.append(rec)
        steps.append(step)
    return tuple(key), steps, dev


def _adam_table(key, dev):
    """device table (SaAdamRec per tensor) and block -> (tensor, chunk) map of one param group"""
    arr = (L.SaAdamRec * len(key))()
    blocks = []
    for t, (r, (p, m, v, step, n, gbase, goff)) in enumerate(zip(arr, key)):
        r.p, r.m, r.v, r.step, r.n, r.gbase = p, m, v, step, n, gbase
        r.g, r.goff = (goff, 0) if gbase < 0 else (None, goff)
        blocks.extend((t, c) for c in range(-(-n // L.ADAM_CHUNK)))
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    bmap = torch.tensor(blocks, dtype=torch.int32).to(dev)
    return table, bmap, len(key), len(blocks)


def adam_step(opt, flats=None):
    """optimizer.step() of a plain torch.optim.Adam(fused=True) with its arithmetic in one launch per param group
    (sa_adam_step: torch 2.10's fused fp32 update, same bits); torch keeps owning param_groups, state and lr, and
    advances the step counters (_foreach_add_) as its own step() does.  Returns False, having done nothing, for
    every case the kernel does not cover -- the caller then runs opt.step().

    flats: flat gradient buckets (a model's _last_flats).  A gradient that is a view of one is recorded as
    (bucket, offset), so buckets that every backward allocates anew change a launch argument and the cached table
    stays.  A table that has to be rebuilt while a hipGraph is being captured is a case for torch's step()."""
    if not _adam_plain(opt):
        return False
    flats = list(flats or ())[:L.FLATS_MAX]
    spans = [(f.data_ptr(), f.data_ptr() + 4 * f.numel()) for f in flats]
    cache = opt.__dict__.setdefault("_sa_adam_tables", {})
    # a captured launch reads its table on every replay: those tables stay alive (and findable) for the optimizer's
    # lifetime, whatever later steps put into the one-entry cache
    captured = opt.__dict__.setdefault("_sa_adam_captured", [])
    capturing = torch.cuda.is_current_stream_capturing()
    plans = []
    for gi, group in enumerate(opt.param_groups):
        plan = _adam_group(opt, group, spans)
        if plan is None:
            return False
        key, steps, dev = plan
        if not key:
            continue
        ent = cache.get(gi)
        if ent is None or ent[0] != key:
            ent = next((e for e in captured if e[0] == key), None)
            if ent is None:
                if capturing:
                    return False
                ent = (key,) + _adam_table(key, dev)
            cache[gi] = ent
        plans.append((group, steps, ent))
    if capturing:
        captured.extend(ent for _, _, ent in plans if not any(ent is e for e in captured))
    bases = L.SaFlats()
    bases.n = len(flats)
    for d, (lo, hi) in zip(bases.f, spans):
        d.p, d.n = lo, (hi - lo) // 4
    lib = L.load()
    for group, steps, (_, table, bmap, nt, nblocks) in plans:
        torch._foreach_add_(steps, 1)
        lr = group["lr"]
        lr_dev, lr_host = (_f(lr), 0.0) if torch.is_tensor(lr) else (None, float(lr))
        b1, b2 = group["betas"]
        L.check(lib.sa_adam_step(_f(table), nt, _f(bmap), nblocks, C.byref(bases), lr_dev, C.c_double(lr_host),
                                 C.c_double(b1), C.c_double(b2), C.c_double(group["eps"]), L.stream()), "sa_adam_step")
    return True


# ---- waveform augmentation (csrc/sa_augment.hip; augment.py) ----
def _aug_in(t, what, dtype=torch.float32, shape=None, family="augmentation"):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.SaHipError(f"{what}: the {family} kernels take GPU tensors (no CPU fallback)")
    if t.dtype != dtype:
        raise L.SaHipError(f"{what}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.SaHipError(f"{what}: expected a contiguous tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise L.SaHipError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def wav_abs_sums(wav, noise=None):
    """per-row sum |x| of wav [B, L] and, if given, of noise [B, L]: fp64 [2, B] (row 1 unwritten without noise)"""
    if _aug_in(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, L] with B, L >= 1, got {tuple(wav.shape)}")
    B, Lw = wav.shape
    if noise is not None:
        _aug_in(noise, "noise", shape=(B, Lw))
    sums = torch.empty(2, B, dtype=torch.float64, device=wav.device)
    L.check(L.load().sa_wav_abs_sums(_f(wav), _f(noise), B, Lw, _f(sums), L.stream()), "sa_wav_abs_sums")
    return sums


def noise_scales(sums, lens, snr, Lw):
    """scales [B, 2] = (1 - f, f amp_clean / (amp_noise + 1e-14)) from wav_abs_sums' sums, the relative lengths
    and the SNRs in dB (both fp32 [B] on the device); fp64 on the device, rounded once"""
    B = _aug_in(lens, "lens").numel()
    _aug_in(sums, "sums", torch.float64, (2, B))
    _aug_in(snr, "snr", shape=(B,))
    scales = torch.empty(B, 2, dtype=torch.float32, device=sums.device)
    L.check(L.load().sa_noise_scales(_f(sums), _f(lens), _f(snr), B, int(Lw), _f(scales), L.stream()),
            "sa_noise_scales")
    return scales


def wav_augment(wav, noise, scales, plan_words, R, Lp, S_in, S_out, W, first_min, first_max):
    """the fused pass (one launch): wav [B, L] -> [R, Lp]; R = 2 B takes noise [B, L] and scales [B, 2].
    plan_words: the device copy of augment.Plan.words()."""
    if _aug_in(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, L] with B, L >= 1, got {tuple(wav.shape)}")
    B, Lw = wav.shape
    if R not in (B, 2 * B):
        raise L.SaHipError(f"R = {R}: the output has B = {B} rows, or 2 B with noise rows")
    if R == 2 * B:
        _aug_in(noise, "noise", shape=(B, Lw))
        _aug_in(scales, "scales", shape=(B, 2))
    else:
        noise = scales = None
    from . import augment
    need = S_out + S_out * W + 101 + R * (1 + 2 * augment.max_chunks())
    if _aug_in(plan_words, "plan", torch.int32).numel() < need:
        raise L.SaHipError(f"plan: {plan_words.numel()} words, the geometry needs {need}")
    out = torch.empty(R, Lp, dtype=torch.float32, device=wav.device)
    L.check(L.load().sa_wav_augment(_f(wav), _f(noise), _f(scales), _f(plan_words), B, Lw, R, int(Lp), int(S_in),
                                    int(S_out), int(W), int(first_min), int(first_max), _f(out), L.stream()),
            "sa_wav_augment")
    return out


# ---- SpecAugment of the input features (csrc/sa_specaug.hip; specaug.py) ----
SPECAUG_TILE = 32          # output frames per workgroup of sa_specaug_warp_sums / sa_specaug_fill


def _specaug_shape(x, what):
    if _aug_in(x, what).dim() != 3:
        raise L.SaHipError(f"{what}: expected [B, T, F], got {tuple(x.shape)}")
    B, T, F = x.shape
    if B < 1 or B > 65535 or T < 1 or F < 4 or F % 4 or F > 128:
        raise L.SaHipError(f"{what}: [B, T, F] = {tuple(x.shape)} -- B in 1..65535, T >= 1, F a multiple of 4 up to 128")
    if x.data_ptr() % 16:
        raise L.SaHipError(f"{what}: expected 16-byte aligned storage")
    return B, T, F


def _specaug_plan(words, B, T):
    from . import specaug
    need = specaug.plan_words(B, T)
    if _aug_in(words, "plan", torch.int32).numel() < need:
        raise L.SaHipError(f"plan: {words.numel()} words, the geometry needs {need}")


def specaug_warp_sums(x, plan_words):
    """x [B, T, F] -> (the warped features, a new tensor; part [tiles * B, 2] fp64: per workgroup the sum of its
    values and of those in frequency-masked columns).  plan_words: the device copy of specaug.Plan.words()."""
    B, T, F = _specaug_shape(x, "x")
    _specaug_plan(plan_words, B, T)
    out = torch.empty_like(x)
    part = torch.empty(-(-T // SPECAUG_TILE) * B, 2, dtype=torch.float64, device=x.device)
    L.check(L.load().sa_specaug_warp_sums(_f(x), _f(plan_words), B, T, F, _f(out), _f(part), L.stream()),
            "sa_specaug_warp_sums")
    return out, part


def specaug_finalize(part, plan_words, B, T, F):
    """vals [2] fp32 = (val_f, val_t), the fill values of the frequency and of the time masks, from the partial sums"""
    B, T, F = int(B), int(T), int(F)
    _aug_in(part, "part", torch.float64, (-(-T // SPECAUG_TILE) * B, 2))
    _specaug_plan(plan_words, B, T)
    vals = torch.empty(2, dtype=torch.float32, device=part.device)
    L.check(L.load().sa_specaug_finalize(_f(part), _f(plan_words), B, T, F, _f(vals), L.stream()),
            "sa_specaug_finalize")
    return vals


def specaug_fill(out, plan_words, vals):
    """stores vals on the masked cells of out [B, T, F] (in place; out is what specaug_warp_sums returned) -> out"""
    B, T, F = _specaug_shape(out, "out")
    _specaug_plan(plan_words, B, T)
    _aug_in(vals, "vals", shape=(2,))
    L.check(L.load().sa_specaug_fill(_f(plan_words), _f(vals), B, T, F, _f(out), L.stream()), "sa_specaug_fill")
    return out


# ---- Griffin-Lim inversion (csrc/sa_vocoder.hip; vocoder.py) ----
GL_MAX_B, GL_MAX_T = 65535, 1 << 23        # grid.y; 160 T + 400 stays an int


_gl_in = functools.partial(_aug_in, family="vocoder")


def _gl_spec(t, what, dtype, family_in=_gl_in, t_min=2):
    """(B, T) of t [B, T, 201] as the kernels of one family take it; t_min None: the caller checks the extents"""
    if family_in(t, what, dtype).dim() != 3 or t.shape[2] != 201:
        raise L.SaHipError(f"{what}: expected [B, T, 201], got {tuple(t.shape)}")
    B, T, _ = t.shape
    if t_min is not None and (B < 1 or B > GL_MAX_B or T < t_min or T > GL_MAX_T):
        raise L.SaHipError(f"{what}: [B, T] = [{B}, {T}] -- B in 1..{GL_MAX_B} (a grid extent), T in "
                           f"{t_min}..{GL_MAX_T}")
    return B, T


def _gl_tables(window, twiddle):
    _gl_in(window, "window", shape=(400,))
    _gl_in(twiddle, "twiddle", shape=(800,))


def mel_to_mag(x, mean, std, M, frames=None):
    """normalised log-Mel features x [B, Tf, 80] -> linear magnitudes S [B, frames, 201] = sqrt(max(0, p M)),
    p = 10^((x std + mean) / 10); mean, std [80]; M [80, 201] (vocoder.mel_pinv(), fp32).  frames <= Tf drops
    padding frames, which are not read."""
    if _gl_in(x, "x").dim() != 3 or x.shape[2] != 80:
        raise L.SaHipError(f"x: expected [B, Tf, 80], got {tuple(x.shape)}")
    B, Tf, _ = x.shape
    T = Tf if frames is None else int(frames)
    if B < 1 or B > GL_MAX_B or T < 1 or T > Tf or T > GL_MAX_T:
        raise L.SaHipError(f"x: [B, Tf] = [{B}, {Tf}], frames = {T} -- B in 1..{GL_MAX_B}, frames in 1..Tf")
    _gl_in(mean, "mean", shape=(80,))
    _gl_in(std, "std", shape=(80,))
    _gl_in(M, "M", shape=(80, 201))
    S = torch.empty(B, T, 201, dtype=torch.float32, device=x.device)
    L.check(L.load().sa_mel_to_mag(_f(x), _f(mean), _f(std), _f(M), B, T, Tf, _f(S), L.stream()), "sa_mel_to_mag")
    return S


def gl_istft(C, window, twiddle):
    """C complex64 [B, T, 201] -> y [B, (T - 1) 160] with the semantics of torch.istft(center=True, length=N);
    window [400], twiddle [800] (vocoder.tables)"""
    B, T = _gl_spec(C, "C", torch.complex64)
    _gl_tables(window, twiddle)
    y = torch.empty(B, (T - 1) * 160, dtype=torch.float32, device=C.device)
    L.check(L.load().sa_gl_istft(_f(C), _f(window), _f(twiddle), B, T, _f(y), L.stream()), "sa_gl_istft")
    return y


def gl_project(y, S, Tprev, m, window, twiddle):
    """one projection and phase update: R = STFT(y), A = R - m Tprev, C_new = S A / (|A| + 1e-16) -> (C_new, R),
    both complex64 [B, T, 201], new tensors.  y [B, (T - 1) 160]; S fp32 and Tprev complex64 [B, T, 201];
    m = momentum / (1 + momentum), rounded to fp32."""
    B, T = _gl_spec(S, "S", torch.float32)
    _gl_in(Tprev, "Tprev", torch.complex64, (B, T, 201))
    _gl_in(y, "y", shape=(B, (T - 1) * 160))
    _gl_tables(window, twiddle)
    Cn, R = torch.empty_like(Tprev), torch.empty_like(Tprev)
    L.check(L.load().sa_gl_project(_f(y), _f(S), _f(Tprev), C.c_float(float(m)), _f(window), _f(twiddle), B, T,
                                   _f(Cn), _f(R), L.stream()), "sa_gl_project")
    return Cn, R


# ---- pitch normalisation (csrc/sa_pitch.hip; pitchnorm.py) ----
YIN_HOP, YIN_TMAX = 160, 266
PN_MAX_N = 1 << 30

_pn_in = functools.partial(_aug_in, family="pitch")


def _pn_rows(t, what, dtype=torch.float32):
    if _pn_in(t, what, dtype).dim() != 2 or t.numel() == 0:
        raise L.SaHipError(f"{what}: expected [B, N] with B, N >= 1, got {tuple(t.shape)}")
    B, N = t.shape
    if B > GL_MAX_B or N > PN_MAX_N:
        raise L.SaHipError(f"{what}: [B, N] = [{B}, {N}] -- B up to {GL_MAX_B} (a grid extent), N up to {PN_MAX_N}")
    return B, N


def yin_f0(wav, threshold=0.15, return_dprime=False):
    """wav [B, N] -> f0 [B, N // 160 + 1] in Hz, 0 where unvoiced (sa_yin_f0).  return_dprime: also the cumulative
    mean normalised difference d' [B, T, 267] the decision was made on (tests)."""
    B, N = _pn_rows(wav, "wav")
    T = N // YIN_HOP + 1
    f0 = torch.empty(B, T, dtype=torch.float32, device=wav.device)
    dp = torch.empty(B, T, YIN_TMAX + 1, dtype=torch.float32, device=wav.device) if return_dprime else None
    L.check(L.load().sa_yin_f0(_f(wav), B, N, C.c_float(float(threshold)), _f(f0), _f(dp), L.stream()), "sa_yin_f0")
    return (f0, dp) if return_dprime else f0


def pitch_ratio(f0, lens, N, target_hz=170.0, r_min=0.5, r_max=2.0, min_voiced=5):
    """f0 [B, T], relative lengths lens [B] (fp32, device), N samples per row -> (ratio fp32 [B], mean fp32 [B],
    voiced int32 [B]): clamp(target / mean voiced f0) over the frames of round(lens N) samples, 1 under min_voiced"""
    B, T = _pn_rows(f0, "f0")
    _pn_in(lens, "lens", shape=(B,))
    N = int(N)
    if N < 1 or N > PN_MAX_N or T > GL_MAX_T:
        raise L.SaHipError(f"pitch_ratio: N = {N} in 1..{PN_MAX_N} and T = {T} up to {GL_MAX_T} expected")
    if not (float(target_hz) > 0.0 and 0.5 <= float(r_min) <= float(r_max) <= 2.0):
        raise L.SaHipError(f"pitch_ratio: target {target_hz} > 0 and 0.5 <= r_min {r_min} <= r_max {r_max} <= 2 expected")
    ratio = torch.empty(B, dtype=torch.float32, device=f0.device)
    mean = torch.empty(B, dtype=torch.float32, device=f0.device)
    voiced = torch.empty(B, dtype=torch.int32, device=f0.device)
    L.check(L.load().sa_pitch_ratio(_f(f0), _f(lens), B, T, N, C.c_float(float(target_hz)), C.c_float(float(r_min)),
                                    C.c_float(float(r_max)), int(min_voiced), _f(ratio), _f(mean), _f(voiced),
                                    L.stream()), "sa_pitch_ratio")
    return ratio, mean, voiced


def pitch_stretch_mag(R, ratio, Tout):
    """R complex64 [B, T, 201], ratio fp32 [B] -> S fp32 [B, Tout, 201]: |R| read at t' / r_b between its frames for
    t' < ceil((T - 1) r_b) + 1, zero from there on"""
    B, T = _gl_spec(R, "R", torch.complex64)
    _pn_in(ratio, "ratio", shape=(B,))
    Tout = int(Tout)
    if Tout < 1 or Tout > GL_MAX_T:
        raise L.SaHipError(f"pitch_stretch_mag: Tout = {Tout} in 1..{GL_MAX_T} expected")
    S = torch.empty(B, Tout, 201, dtype=torch.float32, device=R.device)
    L.check(L.load().sa_pitch_stretch_mag(_f(R), _f(ratio), B, T, Tout, _f(S), L.stream()), "sa_pitch_stretch_mag")
    return S


def pitch_resample(y, ratio, n_valid, Nout):
    """y [B, Nin], ratio fp32 [B], n_valid int32 [B] -> out [B, Nout]: the windowed-sinc read of y at n r_b for
    n < n_valid_b, zero from there on (sa_pitch_resample)"""
    B, Nin = _pn_rows(y, "y")
    _pn_in(ratio, "ratio", shape=(B,))
    _pn_in(n_valid, "n_valid", torch.int32, (B,))
    Nout = int(Nout)
    if Nout < 1 or Nout > PN_MAX_N // 2:
        raise L.SaHipError(f"pitch_resample: Nout = {Nout} in 1..{PN_MAX_N // 2} expected")
    out = torch.empty(B, Nout, dtype=torch.float32, device=y.device)
    L.check(L.load().sa_pitch_resample(_f(y), _f(ratio), _f(n_valid), B, Nin, Nout, _f(out), L.stream()),
            "sa_pitch_resample")
    return out


# ---- phase-vocoder resynthesis (csrc/sa_phasevoc.hip; pitchnorm.py) ----
_pv_in = functools.partial(_aug_in, family="phase-vocoder")


def _pv_dims(who, R, Tout):
    B, T = _gl_spec(R, "R", torch.complex64, _pv_in, None)
    Tout = int(Tout)
    if B < 1 or B > GL_MAX_B or T < 2 or T > GL_MAX_T or Tout < 1 or Tout > GL_MAX_T:
        raise L.SaHipError(f"{who}: [B, T] = [{B}, {T}], Tout = {Tout} -- B in 1..{GL_MAX_B} (a grid extent), T in "
                           f"2..{GL_MAX_T}, Tout in 1..{GL_MAX_T}")
    return B, T, Tout


def _pv_launch(entry, R, mags, steer, B, T, Tout, return_phase):
    """the output, the workspace and the call of sa_pv_synth and sa_pv_synth_map; steer: what places the frames"""
    lib = L.load()
    Cx = torch.empty(B, Tout, 201, dtype=torch.complex64, device=R.device)
    phase = torch.empty(B, Tout, 201, dtype=torch.float64, device=R.device) if return_phase else None
    ws = torch.empty(lib.sa_pv_workspace_bytes(B, Tout) // 8, dtype=torch.float64, device=R.device)
    L.check(getattr(lib, entry)(_f(R), _f(mags), *(_f(t) for t in steer), B, T, Tout, _f(Cx), _f(phase), _f(ws),
                                L.stream()), entry)
    return (Cx, phase) if return_phase else Cx


def pv_synth(R, ratio, Tout, S=None, return_phase=False):
    """R complex64 [B, T, 201] (vocoder.stft of the padded waveform), ratio fp32 [B] -> C complex64 [B, Tout, 201]: the
    stretch of pitch_stretch_mag with R's own phases carried through it -- frame t' < ceil((T - 1) r_b) + 1 has the
    phase theta[0] + sum_{s < t'} (theta[i_s + 1] - theta[i_s]) and the magnitude S[b, t'] (fp32 [B, Tout, 201], e.g.
    env_warp's output) or, without S, what pitch_stretch_mag gives bit for bit; zero from there on (sa_pv_synth).
    return_phase: also the phases in turns, fp64 [B, Tout, 201] (tests).  Everything stays on the device."""
    B, T, Tout = _pv_dims("pv_synth", R, Tout)
    _pv_in(ratio, "ratio", shape=(B,))
    if S is not None:
        _pv_in(S, "S", shape=(B, Tout, 201))
    return _pv_launch("sa_pv_synth", R, S, (ratio,), B, T, Tout, return_phase)


# ---- spectral envelope and formant warp (csrc/sa_envelope.hip; pitchnorm.py) ----
ENV_NC_MAX = 64
LN10_OVER_20 = 0.11512925464970229       # dB -> natural log of an amplitude ratio

_env_in = functools.partial(_aug_in, family="envelope")


def _env_warp(who, S, q, per_frame, n_c, floor_rel, max_gain_db, return_env):
    B, T = _gl_spec(S, "S", torch.float32, _env_in, 1)
    _env_in(q, "q", shape=(B, T) if per_frame else (B,))
    n_c = int(n_c)
    if not 1 <= n_c <= ENV_NC_MAX:
        raise L.SaHipError(f"{who}: n_c = {n_c} in 1..{ENV_NC_MAX} expected")
    if not 0.0 < float(floor_rel) < 1.0:
        raise L.SaHipError(f"{who}: floor_rel = {floor_rel} in (0, 1) expected")
    if not float(max_gain_db) > 0.0:
        raise L.SaHipError(f"{who}: max_gain_db = {max_gain_db} > 0 expected")
    out = torch.empty_like(S)
    env = torch.empty_like(S) if return_env else None
    L.check(getattr(L.load(), "sa_" + who)(_f(S), _f(q), B, T, n_c, C.c_float(float(floor_rel)),
                                           C.c_float(float(max_gain_db) * LN10_OVER_20), _f(out), _f(env), L.stream()),
            "sa_" + who)
    return (out, env) if return_env else out


def env_warp(S, q, n_c=30, floor_rel=1e-4, max_gain_db=40.0, return_env=False):
    """magnitudes S fp32 [B, T, 201], warp factors q fp32 [B] -> out [B, T, 201] = S exp(g), g = clamp(E(min(pi, q w_k))
    - E(w_k), +-max_gain_db ln 10 / 20), E the cepstral envelope of ln max(S, floor_rel max S, 1e-10) liftered to
    n_c coefficients (sa_env_warp).  return_env: also E(w_k) [B, T, 201] (tests)."""
    return _env_warp("env_warp", S, q, False, n_c, floor_rel, max_gain_db, return_env)


def env_warp_frames(S, q, n_c=30, floor_rel=1e-4, max_gain_db=40.0, return_env=False):
    """env_warp with warp factors q fp32 [B, T], one per frame (sa_env_warp_frames): for q constant
    along t, env_warp's bits"""
    return _env_warp("env_warp_frames", S, q, True, n_c, floor_rel, max_gain_db, return_env)


# ---- F0-contour pitch modification (csrc/sa_contour.hip; pitchnorm.py) ----
CT_SMOOTH_MAX = 8                          # sa_contour_dim(1)
CT_RHO_ONE, CT_Q_ONE = 1 << 16, 1 << 17    # ratio 1 in rho_q; one input frame in Q

_ct_in = functools.partial(_aug_in, family="contour")


def _ct_tables(rho_q, Q, B, T):
    _ct_in(rho_q, "rho_q", torch.int32, (B, T))
    _ct_in(Q, "Q", torch.int64, (B, T))


def pitch_contour(f0, lens, N, target_hz=170.0, gamma=1.0, smooth=2, r_min=0.5, r_max=2.0, min_voiced=5):
    """f0 [B, T] (yin_f0 of the padded waveform), relative lengths lens [B], N samples per row -> (rho_q int32 [B, T],
    Q int64 [B, T], Tq int32 [B], mean fp32 [B], voiced int32 [B]): the per-frame ratio that moves the contour to
    target + gamma (f0 - mean), in units of 2^-16, its time map in units of 2^-17 frames and the frames T'_b the
    stretch gives; mean and voiced as pitch_ratio's (sa_pitch_contour)"""
    B, T = _pn_rows(f0, "f0")
    _ct_in(lens, "lens", shape=(B,))
    N, smooth = int(N), int(smooth)
    if N < 1 or N > PN_MAX_N or T < 2 or T > GL_MAX_T:
        raise L.SaHipError(f"pitch_contour: N = {N} in 1..{PN_MAX_N} and T = {T} in 2..{GL_MAX_T} expected")
    if not (float(target_hz) > 0.0 and 0.5 <= float(r_min) <= float(r_max) <= 2.0):
        raise L.SaHipError(f"pitch_contour: target {target_hz} > 0 and 0.5 <= r_min {r_min} <= r_max {r_max} <= 2 "
                           "expected")
    if not 0.0 <= float(gamma) <= 2.0 or not 0 <= smooth <= CT_SMOOTH_MAX:
        raise L.SaHipError(f"pitch_contour: gamma {gamma} in [0, 2] and smooth {smooth} in 0..{CT_SMOOTH_MAX} expected")
    dev = f0.device
    rho_q = torch.empty(B, T, dtype=torch.int32, device=dev)
    Q = torch.empty(B, T, dtype=torch.int64, device=dev)
    Tq = torch.empty(B, dtype=torch.int32, device=dev)
    mean = torch.empty(B, dtype=torch.float32, device=dev)
    voiced = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(L.load().sa_pitch_contour(_f(f0), _f(lens), B, T, N, C.c_float(float(target_hz)), C.c_float(float(gamma)),
                                      smooth, C.c_float(float(r_min)), C.c_float(float(r_max)), int(min_voiced),
                                      _f(rho_q), _f(Q), _f(Tq), _f(mean), _f(voiced), L.stream()), "sa_pitch_contour")
    return rho_q, Q, Tq, mean, voiced


def pv_synth_map(R, rho_q, Q, Tout, M=None, return_phase=False):
    """pv_synth with the stretch positions of a time map (pitch_contour's rho_q and Q, [B, T]) in place of a ratio's;
    M fp32 [B, T, 201]: magnitudes ON THE INPUT GRID (e.g. env_warp_frames' output), mixed as the stretch mixes |R|;
    without M, |R| (sa_pv_synth_map).  Everything stays on the device."""
    B, T, Tout = _pv_dims("pv_synth_map", R, Tout)
    _ct_tables(rho_q, Q, B, T)
    if M is not None:
        _pv_in(M, "M", shape=(B, T, 201))
    return _pv_launch("sa_pv_synth_map", R, M, (rho_q, Q), B, T, Tout, return_phase)


def pitch_resample_map(y, rho_q, Q, n_valid, Nout):
    """y [B, Nin], the time map (rho_q, Q: [B, T]), n_valid int32 [B] -> out [B, Nout]: the windowed-sinc read of y at
    the positions the map gives output sample n < n_valid_b, zero from there on (sa_pitch_resample_map)"""
    B, Nin = _pn_rows(y, "y")
    if not torch.is_tensor(rho_q) or rho_q.dim() != 2:
        raise L.SaHipError("rho_q: expected [B, T]")
    T = rho_q.shape[1]
    _ct_tables(rho_q, Q, B, T)
    _ct_in(n_valid, "n_valid", torch.int32, (B,))
    Nout = int(Nout)
    if Nout < 1 or Nout > PN_MAX_N // 2 or T < 2 or T > GL_MAX_T:
        raise L.SaHipError(f"pitch_resample_map: Nout = {Nout} in 1..{PN_MAX_N // 2} and T = {T} in 2..{GL_MAX_T} "
                           "expected")
    out = torch.empty(B, Nout, dtype=torch.float32, device=y.device)
    L.check(L.load().sa_pitch_resample_map(_f(y), _f(rho_q), _f(Q), _f(n_valid), B, Nin, Nout, T, _f(out),
                                           L.stream()), "sa_pitch_resample_map")
    return out


# ---- McAdams-coefficient anonymisation (csrc/sa_mcadams.hip; mcadams.py) ----
MC_W, MC_H, MC_CHUNK = 320, 160, 4096      # sa_mcadams_dim(0), (1), (6)

_mc_in = functools.partial(_aug_in, family="McAdams")


def mcadams_frames(N):
    """T = (N + 159) // 160 + 1: the frames of N samples"""
    return (int(N) + MC_H - 1) // MC_H + 1


def mcadams_workspace(B, N, device):
    """the workspace sa_mcadams takes: [B][T][320] fp32 frames, then the level sums (fp64 [B][ceil(N / 4096)][2]) and
    gains (fp64 [B]), as one 8-byte-aligned buffer"""
    words = B * mcadams_frames(N) * MC_W // 2 + 2 * B * (-(-int(N) // MC_CHUNK)) + B       # (320 B T is even)
    return torch.empty(words, dtype=torch.float64, device=device)


def _fr_bounds(B, N):
    if B > GL_MAX_B or N > PN_MAX_N or mcadams_frames(N) > GL_MAX_T:
        raise L.SaHipError(f"wav: [B, N] = [{B}, {N}] -- B up to {GL_MAX_B} (a grid extent), N up to {PN_MAX_N}")


def _fr_call(entry, wav, other, n_valid, level, return_status, *, check, bounds, workspace, what, per_sample=False):
    """what mcadams, pole_warp and srcfilt_synth share: the [B, N] check of wav (``check``: the family's _aug_in),
    ``bounds(B, N)``, the second input ``other`` (named ``what``; [B, N] when per_sample, [B] otherwise) and n_valid,
    the outputs, the workspace and the call of ``entry``"""
    if check(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, N] with B, N >= 1, got {tuple(wav.shape)}")
    B, N = wav.shape
    bounds(B, N)
    check(other, what, shape=(B, N) if per_sample else (B,))
    check(n_valid, "n_valid", torch.int32, (B,))
    out = torch.empty_like(wav)
    gain = torch.empty(B, dtype=torch.float32, device=wav.device)
    status = torch.empty(B, mcadams_frames(N), dtype=torch.int32, device=wav.device) if return_status else None
    ws = workspace(B, N, wav.device)
    L.check(getattr(L.load(), entry)(_f(wav), _f(other), _f(n_valid), B, N, int(bool(level)), _f(out), _f(ws),
                                     _f(status), _f(gain), L.stream()), entry)
    return (out, gain, status) if return_status else (out, gain)


def mcadams(wav, alpha, n_valid, level=True, return_status=False):
    """wav fp32 [B, N], alpha fp32 [B], n_valid int32 [B] -> (out fp32 [B, N], gain fp32 [B]): every frame's LPC poles
    moved from angle phi to phi^alpha_b and the frame re-synthesised from its own residual; ``level``: the RMS over
    the samples below n_valid_b brought back to the input's (sa_mcadams).  return_status: also int32 [B, T], 0 a frame
    that was transformed, 1 a silent one, 2 one kept as it was (tests, reports)."""
    return _fr_call("sa_mcadams", wav, alpha, n_valid, level, return_status, check=_mc_in, bounds=_fr_bounds,
                    workspace=mcadams_workspace, what="alpha")


# ---- STOI / ESTOI intelligibility scoring (csrc/sa_stoi.hip) ----
STOI_W, STOI_H, STOI_SEG, STOI_HALF, STOI_MAX_N = 256, 128, 30, 80, 1 << 24      # sa_stoi_dim(1), (2), (5), (6) // 2

_stoi_in = functools.partial(_aug_in, family="STOI")
_stoi_taps = {}


def stoi_taps(device):
    """h[k + 80] = (5/8) sinc(k/8) I0(5 sqrt(1 - (k/80)^2)) / I0(5), k = -80..80, fp64: built on the host once per
    device (the 16 kHz -> 10 kHz Kaiser windowed sinc)"""
    device = torch.device(device)
    t = _stoi_taps.get(device)
    if t is None:
        k = torch.arange(-STOI_HALF, STOI_HALF + 1, dtype=torch.float64)
        five = torch.tensor(5.0, dtype=torch.float64)
        h = 0.625 * torch.sinc(k / 8.0) * torch.special.i0(5.0 * torch.sqrt(1.0 - (k / STOI_HALF) ** 2))
        t = _stoi_taps[device] = (h / torch.special.i0(five)).to(device)
    return t


def stoi_frames(N):
    """(M, F): the 10 kHz samples and the frames of N samples at 16 kHz, as the workspace is laid out"""
    M = (5 * int(N) + 7) // 8
    return M, ((M - STOI_W) // STOI_H + 1 if M >= STOI_W else 1)


def stoi_workspace(B, N, device):
    """the workspace sa_stoi takes: 8 B (2 M + 33 F) + 4 B (F + 2) bytes as one 8-byte-aligned buffer"""
    M, F = stoi_frames(N)
    return torch.empty(B * (2 * M + 33 * F) + (B * (F + 2) + 1) // 2, dtype=torch.float64, device=device)


def stoi(ref, deg, n_valid, extended=True):
    """ref, deg fp32 [B, N] at 16 kHz, n_valid int32 [B] -> (stoi fp32 [B], estoi fp32 [B] | None, frames int32 [B],
    segments int32 [B]): the short-time objective intelligibility of deg against ref and its extended form over the
    samples below n_valid_b, both 0 where a row has fewer than 30 frames within 40 dB of its loudest (segments = 0).
    Everything stays on the device (sa_stoi)."""
    if _stoi_in(ref, "ref").dim() != 2 or ref.numel() == 0:
        raise L.SaHipError(f"ref: expected [B, N] with B, N >= 1, got {tuple(ref.shape)}")
    B, N = ref.shape
    if B > GL_MAX_B or N > STOI_MAX_N:
        raise L.SaHipError(f"ref: [B, N] = [{B}, {N}] -- B up to {GL_MAX_B} (a grid extent), N up to {STOI_MAX_N}")
    _stoi_in(deg, "deg", shape=(B, N))
    _stoi_in(n_valid, "n_valid", torch.int32, (B,))
    dev = ref.device
    out = torch.empty(B, dtype=torch.float32, device=dev)
    ext = torch.empty(B, dtype=torch.float32, device=dev) if extended else None
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    segments = torch.empty(B, dtype=torch.int32, device=dev)
    ws = stoi_workspace(B, N, dev)
    L.check(L.load().sa_stoi(_f(ref), _f(deg), _f(n_valid), B, N, _f(stoi_taps(dev)), _f(out), _f(ext), _f(frames),
                             _f(segments), _f(ws), L.stream()), "sa_stoi")
    return out, ext, frames, segments


# ---- Viterbi F0 tracking (csrc/sa_f0track.hip; pitchnorm.f0_track) ----
F0V_K, F0V_STATES, F0V_FRAC = 8, 9, 16     # sa_f0v_dim(0), (1), (4)
F0V_TMIN = 40                              # sa_yin_dim(3)
F0V_WEIGHT_MAX = 4.0

_f0v_in = functools.partial(_aug_in, family="F0 tracking")
_f0v_log, _f0v_ws = {}, {}


def f0v_log_table(device):
    """LOG[tau] = rint(log2(max(tau, 1)) 2^16), int32 [267]: computed once in fp64 on the host, kept per device"""
    device = torch.device(device)
    t = _f0v_log.get(device)
    if t is None:
        import numpy as np
        lg = np.rint(np.log2(np.maximum(np.arange(YIN_TMAX + 1), 1).astype(np.float64)) * (1 << F0V_FRAC))
        t = _f0v_log[device] = torch.from_numpy(lg.astype(np.int32)).to(device)
    return t


def _f0v_workspace(B, T, device):
    """psi, uint8 [B, T, 9]: one buffer per device, grown when a call needs more; its contents mean nothing between
    calls"""
    device = torch.device(device)
    ws = _f0v_ws.get(device)
    if ws is None or ws.numel() < B * T * F0V_STATES:
        ws = _f0v_ws[device] = torch.empty(B * T * F0V_STATES, dtype=torch.uint8, device=device)
    return ws


def _f0v_dprime(dprime):
    if _f0v_in(dprime, "dprime").dim() != 3 or dprime.shape[2] != YIN_TMAX + 1 or dprime.numel() == 0:
        raise L.SaHipError(f"dprime: expected [B, T, {YIN_TMAX + 1}] with B, T >= 1, got {tuple(dprime.shape)}")
    B, T, _ = dprime.shape
    if B > GL_MAX_B or T > GL_MAX_T:
        raise L.SaHipError(f"dprime: [B, T] = [{B}, {T}] -- B up to {GL_MAX_B} (a grid extent), T up to {GL_MAX_T}")
    return B, T


def f0_candidates(dprime):
    """dprime fp32 [B, T, 267] (yin_f0's) -> (tau, q) int32 [B, T, 8]: per frame the 8 dips of d' with the smallest
    (q, tau), q = rint(clamp(d', 0, 1) 2^16), in ascending lag; unused slots hold tau = -1, q = 0 (sa_f0_candidates)"""
    B, T = _f0v_dprime(dprime)
    tau = torch.empty(B, T, F0V_K, dtype=torch.int32, device=dprime.device)
    q = torch.empty(B, T, F0V_K, dtype=torch.int32, device=dprime.device)
    L.check(L.load().sa_f0_candidates(_f(dprime), B, T, _f(tau), _f(q), L.stream()), "sa_f0_candidates")
    return tau, q


def f0_viterbi(dprime, tau, q, lens, N, voicing_cost=0.15, switch_cost=0.14, jump_cost=0.35, lag_bias=0.01,
               return_path=False, log_q=None):
    """dprime [B, T, 267], f0_candidates' tau and q, relative lengths lens [B], N samples per row -> f0 fp32 [B, T] in
    Hz along the cheapest path through the candidates and an unvoiced state, 0 where unvoiced and beyond the frames of
    round(lens N) samples (sa_f0_viterbi).  The costs are per unit of d' (voicing, switch) and per octave (jump, lag
    bias), each in [0, 4].  return_path: also path int32 [B, T], the candidate index or -1.  log_q: the int32 [267]
    table of rint(log2(tau) 2^16) to use instead of the cached one (tests)."""
    B, T = _f0v_dprime(dprime)
    _f0v_in(tau, "tau", torch.int32, (B, T, F0V_K))
    _f0v_in(q, "q", torch.int32, (B, T, F0V_K))
    _f0v_in(lens, "lens", shape=(B,))
    if log_q is not None:
        _f0v_in(log_q, "log_q", torch.int32, (YIN_TMAX + 1,))
    N = int(N)
    if N < 1 or N > PN_MAX_N:
        raise L.SaHipError(f"f0_viterbi: N = {N} in 1..{PN_MAX_N} expected")
    costs = [float(voicing_cost), float(switch_cost), float(jump_cost), float(lag_bias)]
    if not all(0.0 <= w <= F0V_WEIGHT_MAX for w in costs):
        raise L.SaHipError(f"f0_viterbi: voicing, switch, jump and lag-bias costs in [0, {F0V_WEIGHT_MAX:g}] expected, "
                           f"got {costs}")
    dev = dprime.device
    log_q = f0v_log_table(dev) if log_q is None else log_q
    path = torch.empty(B, T, dtype=torch.int32, device=dev)
    f0 = torch.empty(B, T, dtype=torch.float32, device=dev)
    L.check(L.load().sa_f0_viterbi(_f(dprime), _f(tau), _f(q), _f(lens), _f(log_q), B, T, N, *(C.c_float(w) for w in costs),
                                   _f(_f0v_workspace(B, T, dev)), _f(path), _f(f0), L.stream()), "sa_f0_viterbi")
    return (f0, path) if return_path else f0


# ---- pitch-correlation scoring (csrc/sa_prosody.hip) ----
F0CMP_MAX_LAG, F0CMP_MAX_T = 32, (1 << 24) // 160 + 1       # sa_f0cmp_dim(1); the frames of 2^24 samples

_f0cmp_in = functools.partial(_aug_in, family="F0 comparison")


def f0_compare(f0_ref, f0_deg, frames, max_lag=8, min_common=8):
    """f0_ref, f0_deg fp32 [B, T] in Hz (0 or less: unvoiced; two tracks of pitchnorm.f0_track), frames int32 [B] (the
    frames of a row that count, clamped to [0, T]) -> (rho fp32 [B], lag int32 [B], common int32 [B], shift_st fp32 [B],
    dev_st fp32 [B], voicing fp32 [B]): the largest Pearson correlation of the two tracks over the frames voiced in
    both, deg read up to max_lag frames before or after ref; the lag it is found at; the frames it is taken over; the
    mean and the standard deviation of 12 log2(deg / ref) over them, in semitones; the share of frames on which the
    voicing of the two agrees.  A row without a lag of at least min_common common frames and a moving contour in both
    gets rho = lag = common = shift_st = dev_st = 0.  Everything stays on the device (sa_f0_compare)."""
    if _f0cmp_in(f0_ref, "f0_ref").dim() != 2 or f0_ref.numel() == 0:
        raise L.SaHipError(f"f0_ref: expected [B, T] with B, T >= 1, got {tuple(f0_ref.shape)}")
    B, T = f0_ref.shape
    if B > GL_MAX_B or T > F0CMP_MAX_T:
        raise L.SaHipError(f"f0_ref: [B, T] = [{B}, {T}] -- B up to {GL_MAX_B} (a grid extent), T up to {F0CMP_MAX_T}")
    _f0cmp_in(f0_deg, "f0_deg", shape=(B, T))
    _f0cmp_in(frames, "frames", torch.int32, (B,))
    max_lag, min_common = int(max_lag), int(min_common)
    if not 0 <= max_lag <= F0CMP_MAX_LAG or min_common < 2:
        raise L.SaHipError(f"f0_compare: max_lag in 0..{F0CMP_MAX_LAG} and min_common >= 2 expected, got {max_lag} and "
                           f"{min_common}")
    dev = f0_ref.device
    rho, shift, sdev, voicing = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(4))
    lag, common = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    L.check(L.load().sa_f0_compare(_f(f0_ref), _f(f0_deg), _f(frames), B, T, max_lag, min_common, _f(rho), _f(lag),
                                   _f(common), _f(shift), _f(sdev), _f(voicing), L.stream()), "sa_f0_compare")
    return rho, lag, common, shift, sdev, voicing


# ---- mel-cepstral distortion scoring (csrc/sa_mcd.hip) ----
_mcd_in = functools.partial(_aug_in, family="MCD")
_mcd_dims = {"MCD_MAX_BAND": 0, "MCD_MAX_ORDER": 1, "MCD_MAX_MELS": 2, "MCD_MAX_T": 3}


def __getattr__(name):
    """MCD_MAX_BAND, MCD_MAX_ORDER, MCD_MAX_MELS, MCD_MAX_T: sa_mcd_dim(0..3), read from the library on first use"""
    if name in _mcd_dims:
        globals()[name] = L.load().sa_mcd_dim(_mcd_dims[name])
        return globals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def mcd_workspace(B, T_ref, T_deg, order, band, device):
    """the workspace sa_mcd takes: 8 B (K (T_ref + T_deg) + (R + 1) (T_ref + T_deg - 1)) bytes"""
    return torch.empty(B * (order * (T_ref + T_deg) + (band + 1) * (T_ref + T_deg - 1)), dtype=torch.float64,
                       device=device)


def mcd(mel_ref, mel_deg, n_ref, n_deg, order=13, band=16):
    """mel_ref fp32 [B, T_ref, n_mels], mel_deg fp32 [B, T_deg, n_mels] (log-Mel power in dB: features.Fbank(...)(wav)
    .clamped()), n_ref, n_deg int32 [B] (the frames of a row that count, clamped to [0, T]) -> (mcd fp32 [B], mcd_sync
    fp32 [B], frames int32 [B]): the mel-cepstral distortion in dB over the coefficients 1..order along a
    dynamic-time-warping alignment within a band of ``band`` frames, the same figure frame against frame, and
    n_ref + n_deg.  A row with an empty input or with counts more than ``band`` apart gets three zeros.  Everything
    stays on the device (sa_mcd)."""
    if _mcd_in(mel_ref, "mel_ref").dim() != 3 or mel_ref.numel() == 0:
        raise L.SaHipError(f"mel_ref: expected [B, T, n_mels] with B, T, n_mels >= 1, got {tuple(mel_ref.shape)}")
    if _mcd_in(mel_deg, "mel_deg").dim() != 3 or mel_deg.numel() == 0:
        raise L.SaHipError(f"mel_deg: expected [B, T, n_mels] with B, T, n_mels >= 1, got {tuple(mel_deg.shape)}")
    (B, T_ref, n_mels), T_deg = mel_ref.shape, mel_deg.shape[1]
    if (mel_deg.shape[0], mel_deg.shape[2]) != (B, n_mels):
        raise L.SaHipError(f"mel_deg: expected [{B}, T, {n_mels}] as mel_ref has, got {tuple(mel_deg.shape)}")
    _mcd_in(n_ref, "n_ref", torch.int32, (B,))
    _mcd_in(n_deg, "n_deg", torch.int32, (B,))
    this = sys.modules[__name__]
    max_band, max_order, max_mels, max_t = (getattr(this, k) for k in _mcd_dims)
    if B > GL_MAX_B or max(T_ref, T_deg) > max_t or not 2 <= n_mels <= max_mels:
        raise L.SaHipError(f"mel_ref, mel_deg: B up to {GL_MAX_B} (a grid extent), T up to {max_t}, n_mels in "
                           f"2..{max_mels}; got B = {B}, T = {T_ref} and {T_deg}, n_mels = {n_mels}")
    if isinstance(order, bool) or isinstance(band, bool) or not isinstance(order, int) or not isinstance(band, int) \
            or not 1 <= order <= max_order or order >= n_mels or not 0 <= band <= max_band:
        raise L.SaHipError(f"mcd: order in 1..{max_order} and below n_mels = {n_mels}, band in 0..{max_band} expected, "
                           f"got {order!r} and {band!r}")
    dev = mel_ref.device
    out, sync = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2))
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    ws = mcd_workspace(B, T_ref, T_deg, order, band, dev)
    L.check(L.load().sa_mcd(_f(mel_ref), _f(mel_deg), _f(n_ref), _f(n_deg), B, T_ref, T_deg, n_mels, order, band,
                            _f(ws), _f(out), _f(sync), _f(frames), L.stream()), "sa_mcd")
    return out, sync, frames


# ---- TD-PSOLA pitch modification (csrc/sa_psola.hip; pitchnorm.py) ----
PSOLA_MAX_N = 1 << 24
PSOLA_MDIV, PSOLA_JDIV = 30, 15            # sa_psola_dim(6), (7): Mcap = N // 30 + 2, Jcap = N // 15 + 2

_ps_in = functools.partial(_aug_in, family="PSOLA")


def _ps_dims(who, B, N, T):
    if B > GL_MAX_B or not 1 <= N <= PSOLA_MAX_N:
        raise L.SaHipError(f"{who}: [B, N] = [{B}, {N}] -- B up to {GL_MAX_B} (a grid extent), N in 1..{PSOLA_MAX_N}")
    if T not in (N // YIN_HOP + 1, -(-N // YIN_HOP) + 1):
        raise L.SaHipError(f"{who}: f0 has {T} frames; N // 160 + 1 = {N // YIN_HOP + 1} of the waveform (or "
                           f"{-(-N // YIN_HOP) + 1} of the padded one) expected")


def _ps_wav(who, wav, f0, n_valid):
    if _ps_in(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, N] with B, N >= 1, got {tuple(wav.shape)}")
    B, N = wav.shape
    if _ps_in(f0, "f0").dim() != 2 or f0.shape[0] != B:
        raise L.SaHipError(f"f0: expected [{B}, T], got {tuple(f0.shape)}")
    _ps_in(n_valid, "n_valid", torch.int32, (B,))
    _ps_dims(who, B, N, f0.shape[1])
    return B, N, f0.shape[1]


def psola_marks(wav, f0, n_valid):
    """wav fp32 [B, N], f0 fp32 [B, T] in Hz (0 or less: unvoiced; yin_f0's or f0_viterbi's), n_valid int32 [B] ->
    (marks int32 [B, N // 30 + 2], count int32 [B]): the pitch marks of every row, a peak of the waveform per period
    where the frame is voiced and a mark every 80 samples where it is not; entries from count on mean nothing
    (sa_psola_marks)"""
    B, N, T = _ps_wav("psola_marks", wav, f0, n_valid)
    marks = torch.empty(B, N // PSOLA_MDIV + 2, dtype=torch.int32, device=wav.device)
    count = torch.empty(B, dtype=torch.int32, device=wav.device)
    L.check(L.load().sa_psola_marks(_f(wav), _f(f0), _f(n_valid), B, N, T, _f(marks), _f(count), L.stream()),
            "sa_psola_marks")
    return marks, count


def _ps_marks(marks, count, N):
    if _ps_in(marks, "marks", torch.int32).dim() != 2 or marks.numel() == 0:
        raise L.SaHipError(f"marks: expected [B, Mcap], got {tuple(marks.shape)}")
    B = marks.shape[0]
    if marks.shape[1] != N // PSOLA_MDIV + 2:
        raise L.SaHipError(f"marks: expected [{B}, N // 30 + 2 = {N // PSOLA_MDIV + 2}], got {tuple(marks.shape)}")
    _ps_in(count, "count", torch.int32, (B,))
    return B


def psola_plan(marks, count, f0, rho_q, n_valid, *, N):
    """psola_marks' (marks, count), f0 fp32 [B, T], rho_q int32 [B, T] (the ratio per frame in units of 2^-16:
    pitch_contour's, or a constant), n_valid int32 [B], N (by keyword: the samples per row, which no table determines) -> (syn_pos int32 [B, N // 15 + 2], syn_src
    int32 [B, N // 15 + 2], count int32 [B]): where every grain goes and the mark it is cut at; a row under 2 marks
    has count 0 (sa_psola_plan)"""
    N = int(N)
    B = _ps_marks(marks, count, N)
    if _ps_in(f0, "f0").dim() != 2 or f0.shape[0] != B:
        raise L.SaHipError(f"f0: expected [{B}, T], got {tuple(f0.shape)}")
    T = f0.shape[1]
    _ps_in(rho_q, "rho_q", torch.int32, (B, T))
    _ps_in(n_valid, "n_valid", torch.int32, (B,))
    _ps_dims("psola_plan", B, N, T)
    dev = marks.device
    lib = L.load()
    ws = torch.empty(lib.sa_psola_workspace_bytes(B, N) // 8, dtype=torch.int64, device=dev)
    syn_pos, syn_src = (torch.empty(B, N // PSOLA_JDIV + 2, dtype=torch.int32, device=dev) for _ in range(2))
    syn_count = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(lib.sa_psola_plan(_f(marks), _f(count), _f(f0), _f(rho_q), _f(n_valid), B, N, T, _f(ws), _f(syn_pos),
                              _f(syn_src), _f(syn_count), L.stream()), "sa_psola_plan")
    return syn_pos, syn_src, syn_count


def psola_ola(wav, marks, count, syn_pos, syn_src, syn_count, n_valid):
    """the overlap-add of a plan: wav fp32 [B, N] and the tables of psola_marks and psola_plan -> out fp32 [B, N], zero
    from n_valid on; a row without a plan is copied (sa_psola_ola)"""
    if _ps_in(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, N] with B, N >= 1, got {tuple(wav.shape)}")
    B, N = wav.shape
    _ps_dims("psola_ola", B, N, N // YIN_HOP + 1)
    if _ps_marks(marks, count, N) != B:
        raise L.SaHipError(f"marks: expected {B} rows as wav has, got {marks.shape[0]}")
    for name, t in (("syn_pos", syn_pos), ("syn_src", syn_src)):
        _ps_in(t, name, torch.int32, (B, N // PSOLA_JDIV + 2))
    _ps_in(syn_count, "syn_count", torch.int32, (B,))
    _ps_in(n_valid, "n_valid", torch.int32, (B,))
    out = torch.empty_like(wav)
    L.check(L.load().sa_psola_ola(_f(wav), _f(marks), _f(count), _f(syn_pos), _f(syn_src), _f(syn_count), _f(n_valid),
                                  B, N, _f(out), L.stream()), "sa_psola_ola")
    return out


def psola(wav, f0, rho_q, n_valid):
    """wav fp32 [B, N], f0 fp32 [B, T], rho_q int32 [B, T], n_valid int32 [B] -> out fp32 [B, N]: the pitch of every
    voiced frame multiplied by rho_q / 2^16, envelope and duration kept -- marks, plan and overlap-add, three launches
    and nothing copied to the host"""
    B, N, T = _ps_wav("psola", wav, f0, n_valid)
    _ps_in(rho_q, "rho_q", torch.int32, (B, T))
    marks, count = psola_marks(wav, f0, n_valid)
    return psola_ola(wav, marks, count, *psola_plan(marks, count, f0, rho_q, n_valid, N=N), n_valid)


# ---- LPC formant tracking and its comparison (csrc/sa_formants.hip) ----
FORMANT_W, FORMANT_P, FORMANTS = 400, 18, 3                # sa_formant_dim(0), (2), (3)
FORMANT_MAX_N, FORMANT_MAX_T = 1 << 24, (1 << 24) // 160 + 1          # sa_formant_dim(6): the frames of 2^24 samples

_fm_in = functools.partial(_aug_in, family="formant")


def formant_tracks(wav, n_valid, return_bw=False):
    """wav fp32 [B, N] at 16 kHz, n_valid int32 [B] (the samples of a row that count, clamped to [0, N]) -> (freq fp32
    [B, T, 3], status int32 [B, T][, bw fp32 [B, T, 3]]), T = N // 160 + 1 (the frames of yin_f0): per frame of 400
    pre-emphasised, Hamming-windowed samples the three lowest resonances of an order-18 LPC fit between 90 and 5500 Hz
    with a bandwidth up to 700 Hz, in Hz, and their bandwidths; status 0 a frame that has them, 1 a silent one, 2 one
    whose fit or roots failed, 3 one with fewer than three resonances (freq and bw 0 for all but 0).  Everything stays
    on the device (sa_formant_tracks)."""
    if _fm_in(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, N] with B, N >= 1, got {tuple(wav.shape)}")
    B, N = wav.shape
    if B > GL_MAX_B or N > FORMANT_MAX_N:
        raise L.SaHipError(f"wav: [B, N] = [{B}, {N}] -- B up to {GL_MAX_B} (a grid extent), N up to {FORMANT_MAX_N}")
    _fm_in(n_valid, "n_valid", torch.int32, (B,))
    T = N // YIN_HOP + 1
    freq = torch.empty(B, T, FORMANTS, dtype=torch.float32, device=wav.device)
    bw = torch.empty(B, T, FORMANTS, dtype=torch.float32, device=wav.device) if return_bw else None
    status = torch.empty(B, T, dtype=torch.int32, device=wav.device)
    L.check(L.load().sa_formant_tracks(_f(wav), _f(n_valid), B, N, _f(freq), _f(bw), _f(status), L.stream()),
            "sa_formant_tracks")
    return (freq, status, bw) if return_bw else (freq, status)


def formant_compare(F_ref, F_deg, st_ref, st_deg, f0_ref, f0_deg, frames, min_common=8):
    """F_ref, F_deg fp32 [B, T, 3] and st_ref, st_deg int32 [B, T] (two outputs of formant_tracks), f0_ref, f0_deg fp32
    [B, T] in Hz (0 or less: unvoiced; two tracks of pitchnorm.f0_track), frames int32 [B] (the frames of a row that
    count, clamped to [0, T]) -> (med1, med2, med3, r1, r2, r3, shift fp32 [B], common int32 [B]): over the frames with
    status 0 and a voiced F0 in both, the lower median of each formant of F_deg in Hz, the lower median of each
    formant's per-frame ratio F_deg / F_ref, the geometric mean of the three ratios, and the number of those frames.
    A row with fewer than min_common of them gets eight zeros.  Everything stays on the device (sa_formant_compare)."""
    if _fm_in(F_ref, "F_ref").dim() != 3 or F_ref.shape[2] != FORMANTS or F_ref.numel() == 0:
        raise L.SaHipError(f"F_ref: expected [B, T, {FORMANTS}] with B, T >= 1, got {tuple(F_ref.shape)}")
    B, T, _ = F_ref.shape
    if B > GL_MAX_B or T > FORMANT_MAX_T:
        raise L.SaHipError(f"F_ref: [B, T] = [{B}, {T}] -- B up to {GL_MAX_B} (a grid extent), T up to {FORMANT_MAX_T}")
    _fm_in(F_deg, "F_deg", shape=(B, T, FORMANTS))
    _fm_in(st_ref, "st_ref", torch.int32, (B, T))
    _fm_in(st_deg, "st_deg", torch.int32, (B, T))
    _fm_in(f0_ref, "f0_ref", shape=(B, T))
    _fm_in(f0_deg, "f0_deg", shape=(B, T))
    _fm_in(frames, "frames", torch.int32, (B,))
    if isinstance(min_common, bool) or not isinstance(min_common, int) or min_common < 1:
        raise L.SaHipError(f"formant_compare: min_common, a count of frames, 1 or more expected, got {min_common!r}")
    dev = F_ref.device
    med, ratio = (torch.empty(B, FORMANTS, dtype=torch.float32, device=dev) for _ in range(2))
    shift = torch.empty(B, dtype=torch.float32, device=dev)
    common = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(L.load().sa_formant_compare(_f(F_ref), _f(F_deg), _f(st_ref), _f(st_deg), _f(f0_ref), _f(f0_deg), _f(frames),
                                        B, T, min_common, _f(med), _f(ratio), _f(shift), _f(common), L.stream()),
            "sa_formant_compare")
    return (*med.unbind(1), *ratio.unbind(1), shift, common)


# ---- LPC formant normalisation (csrc/sa_formant_norm.hip; formantnorm.py) ----
PW_Q_LOW, PW_Q_HIGH = 0.5, 2.0             # what sa_pole_warp clamps q to on the device
PW_KNEE = 0.85                             # sa_pole_warp_dim(7) / 1000
FORMANT_F_LOW, FORMANT_F_HIGH = 90.0, 5500.0               # the tracker's gate: where a target may lie

_fn_in = functools.partial(_aug_in, family="formant normalisation")


def pole_warp_workspace(B, N, device):
    """the workspace sa_pole_warp takes: sa_mcadams's formula ([B][T][320] fp32 frames, then the level sums and gains
    in fp64), as one 8-byte-aligned buffer"""
    return mcadams_workspace(B, N, device)


def pole_warp(wav, q, n_valid, level=True, return_status=False):
    """wav fp32 [B, N] at 16 kHz, q fp32 [B], n_valid int32 [B] -> (out fp32 [B, N], gain fp32 [B]): every frame's
    complex LPC poles moved from angle phi to q_b phi (piecewise linear above the knee 0.85 pi min(1, 1 / q_b), so that
    (0, pi) maps onto itself) and the frame re-synthesised from its own residual, in sa_mcadams's framing; ``level``:
    the RMS over the samples below n_valid_b brought back to the input's (sa_pole_warp).  return_status: also int32
    [B, T], 0 a frame that was transformed, 1 a silent one, 2 one kept as it was."""
    return _fr_call("sa_pole_warp", wav, q, n_valid, level, return_status, check=_fn_in, bounds=_fr_bounds,
                    workspace=pole_warp_workspace, what="q")


def formant_centre(freq, status, f0, frames, target_hz, q_min=0.8, q_max=1.2, min_frames=8):
    """freq fp32 [B, T, 3] and status int32 [B, T] (one output of formant_tracks), f0 fp32 [B, T] in Hz (0 or less:
    unvoiced) or None (every frame voiced), frames int32 [B] (the frames of a row that count, clamped to [0, T]),
    target_hz (t1, t2, t3) -> (med fp32 [B, 3], q fp32 [B], count int32 [B]): over the frames with status 0 and a
    voiced F0, the lower median of each formant, the ratio clamp((t1 t2 t3 / (m1 m2 m3))^(1/3), q_min, q_max) that
    brings them to the target, and the number of those frames.  A row with fewer than min_frames of them gets med 0,
    q 1 and count 0.  Everything stays on the device (sa_formant_centre)."""
    if _fn_in(freq, "freq").dim() != 3 or freq.shape[2] != FORMANTS or freq.numel() == 0:
        raise L.SaHipError(f"freq: expected [B, T, {FORMANTS}] with B, T >= 1, got {tuple(freq.shape)}")
    B, T, _ = freq.shape
    if B > GL_MAX_B or T > FORMANT_MAX_T:
        raise L.SaHipError(f"freq: [B, T] = [{B}, {T}] -- B up to {GL_MAX_B} (a grid extent), T up to {FORMANT_MAX_T}")
    _fn_in(status, "status", torch.int32, (B, T))
    if f0 is not None:
        _fn_in(f0, "f0", shape=(B, T))
    _fn_in(frames, "frames", torch.int32, (B,))
    try:
        t1, t2, t3 = (float(v) for v in target_hz)
    except (TypeError, ValueError):
        raise L.SaHipError(f"formant_centre: target_hz {target_hz!r}: three frequencies in Hz expected") from None
    if not FORMANT_F_LOW <= t1 < t2 < t3 <= FORMANT_F_HIGH:
        raise L.SaHipError(f"formant_centre: target_hz {target_hz!r}: {FORMANT_F_LOW:g} <= t1 < t2 < t3 <= "
                           f"{FORMANT_F_HIGH:g} expected")
    if not PW_Q_LOW <= float(q_min) <= 1.0 <= float(q_max) <= PW_Q_HIGH:
        raise L.SaHipError(f"formant_centre: {PW_Q_LOW} <= q_min {q_min} <= 1 <= q_max {q_max} <= {PW_Q_HIGH} expected")
    if isinstance(min_frames, bool) or not isinstance(min_frames, int) or min_frames < 1:
        raise L.SaHipError(f"formant_centre: min_frames, a count of frames, 1 or more expected, got {min_frames!r}")
    dev = freq.device
    med = torch.empty(B, FORMANTS, dtype=torch.float32, device=dev)
    q = torch.empty(B, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(L.load().sa_formant_centre(_f(freq), _f(status), _f(f0), _f(frames), B, T, C.c_float(t1), C.c_float(t2),
                                       C.c_float(t3), C.c_float(float(q_min)), C.c_float(float(q_max)), min_frames,
                                       _f(med), _f(q), _f(count), L.stream()), "sa_formant_centre")
    return med, q, count


# ---- LPC source-filter resynthesis (csrc/sa_srcfilt.hip; sourcefilter.py) ----
SRCFILT_MAX_N = 1 << 24
SRCFILT_KDIV = 40                          # sa_srcfilt_dim(7): Kcap = N // 40 + 2
SRCFILT_RHO_ONE = 1 << 16

_sf_in = functools.partial(_aug_in, family="source-filter")


def _sf_dims(who, B, N, T=None):
    if B > GL_MAX_B or not 1 <= N <= SRCFILT_MAX_N:
        raise L.SaHipError(f"{who}: [B, N] = [{B}, {N}] -- B up to {GL_MAX_B} (a grid extent), N in 1..{SRCFILT_MAX_N}")
    if T is not None and T not in (N // YIN_HOP + 1, -(-N // YIN_HOP) + 1):
        raise L.SaHipError(f"{who}: f0 has {T} frames; N // 160 + 1 = {N // YIN_HOP + 1} of the waveform (or "
                           f"{-(-N // YIN_HOP) + 1} of the padded one) expected")


def _sf_track(who, f0, rho_q, n_valid, N):
    if _sf_in(f0, "f0").dim() != 2 or f0.numel() == 0:
        raise L.SaHipError(f"f0: expected [B, T] with B, T >= 1, got {tuple(f0.shape)}")
    B, T = f0.shape
    N = int(N)
    _sf_dims(who, B, N, T)
    if rho_q is not None:
        _sf_in(rho_q, "rho_q", torch.int32, (B, T))
    _sf_in(n_valid, "n_valid", torch.int32, (B,))
    return B, N, T


def _sf_aspiration(who, aspiration):
    if isinstance(aspiration, bool) or not 0.0 <= float(aspiration) <= 1.0:
        raise L.SaHipError(f"{who}: aspiration {aspiration} in 0..1 expected (the noise under the pulses of a voiced "
                           "frame, relative to the noise of an unvoiced one)")
    return float(aspiration)


def srcfilt_workspace(B, N, device):
    """the workspace sa_srcfilt_synth takes (sa_srcfilt_workspace_bytes: sa_mcadams's layout), as one 8-byte-aligned
    buffer"""
    nbytes = L.load().sa_srcfilt_workspace_bytes(int(B), int(N))
    if nbytes < 0:
        raise L.SaHipError(f"srcfilt_workspace: [B, N] = [{B}, {N}] refused")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def srcfilt_pulses(f0, rho_q, n_valid, *, N):
    """f0 fp32 [B, T] in Hz (voiced where 0 < f0 < inf), rho_q int32 [B, T] (the pitch ratio per frame in units of
    2^-16, clamped to [2^15, 2^17]) or None (1 throughout), n_valid int32 [B], N (by keyword: the samples per row) ->
    (pos_q int64 [B, N // 40 + 2] in units of 2^-16 samples, period_q int32 of that shape, count int32 [B]): a pulse
    every 16000 / (f0 rho) samples through the voiced frames; entries from count on mean nothing
    (sa_srcfilt_pulses)"""
    B, N, T = _sf_track("srcfilt_pulses", f0, rho_q, n_valid, N)
    K = N // SRCFILT_KDIV + 2
    pos_q = torch.empty(B, K, dtype=torch.int64, device=f0.device)
    period_q = torch.empty(B, K, dtype=torch.int32, device=f0.device)
    count = torch.empty(B, dtype=torch.int32, device=f0.device)
    L.check(L.load().sa_srcfilt_pulses(_f(f0), _f(rho_q), _f(n_valid), B, N, T, _f(pos_q), _f(period_q), _f(count),
                                       L.stream()), "sa_srcfilt_pulses")
    return pos_q, period_q, count


def srcfilt_excite(f0, pos_q, period_q, count, seed, n_valid, aspiration=0.3, *, N):
    """f0 fp32 [B, T], the table of srcfilt_pulses, seed int32 [B], n_valid int32 [B] -> exc fp32 [B, N]: uniform noise
    in [-1, 1) hashed from (seed_b, n), scaled by ``aspiration`` where the frame is voiced, plus the linearly
    interpolated pulses of amplitude sqrt(period); zero from n_valid on (sa_srcfilt_excite)"""
    B, N, T = _sf_track("srcfilt_excite", f0, None, n_valid, N)
    K = N // SRCFILT_KDIV + 2
    _sf_in(pos_q, "pos_q", torch.int64, (B, K))
    _sf_in(period_q, "period_q", torch.int32, (B, K))
    _sf_in(count, "count", torch.int32, (B,))
    _sf_in(seed, "seed", torch.int32, (B,))
    aspiration = _sf_aspiration("srcfilt_excite", aspiration)
    exc = torch.empty(B, N, dtype=torch.float32, device=f0.device)
    L.check(L.load().sa_srcfilt_excite(_f(f0), _f(pos_q), _f(period_q), _f(count), _f(seed), _f(n_valid), B, N, T,
                                       C.c_float(aspiration), _f(exc), L.stream()), "sa_srcfilt_excite")
    return exc


def srcfilt_synth(wav, exc, n_valid, level=True, return_status=False):
    """wav fp32 [B, N] at 16 kHz, exc fp32 [B, N], n_valid int32 [B] -> (out fp32 [B, N], gain fp32 [B]): every frame
    of sa_mcadams's framing is its own order-20 all-pole filter driven by the windowed excitation, scaled so that the
    frame keeps its prediction-error energy; ``level``: the RMS over the samples below n_valid_b brought back to the
    input's (sa_srcfilt_synth).  return_status: also int32 [B, T'], 0 a frame that was resynthesised, 1 a silent one,
    2 one kept as it was (the fit failed), 3 one without excitation (written as zeros)."""
    return _fr_call("sa_srcfilt_synth", wav, exc, n_valid, level, return_status, check=_sf_in,
                    bounds=functools.partial(_sf_dims, "srcfilt_synth"), workspace=srcfilt_workspace, what="exc",
                    per_sample=True)


def srcfilt(wav, f0, rho_q, seed, n_valid, aspiration=0.3, level=True, return_status=False):
    """wav fp32 [B, N], f0 fp32 [B, T], rho_q int32 [B, T] or None, seed int32 [B], n_valid int32 [B] -> (out fp32
    [B, N], gain fp32 [B], count int32 [B][, status int32 [B, T']]): the waveform's LPC envelope and level under a
    pulse/noise excitation at rho_q / 2^16 times its own pitch -- pulses, excitation and synthesis in a row, and
    nothing copied to the host"""
    if _sf_in(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, N] with B, N >= 1, got {tuple(wav.shape)}")
    B, N = wav.shape
    if _sf_in(f0, "f0").dim() != 2 or f0.shape[0] != B:
        raise L.SaHipError(f"f0: expected [{B}, T], got {tuple(f0.shape)}")
    _sf_track("srcfilt", f0, rho_q, n_valid, N)
    _sf_in(seed, "seed", torch.int32, (B,))
    _sf_aspiration("srcfilt", aspiration)
    pos_q, period_q, count = srcfilt_pulses(f0, rho_q, n_valid, N=N)
    exc = srcfilt_excite(f0, pos_q, period_q, count, seed, n_valid, aspiration, N=N)
    res = srcfilt_synth(wav, exc, n_valid, level, return_status)
    return (res[0], res[1], count) + tuple(res[2:])


# ---- modulation-spectrum smoothing (csrc/sa_modspec.hip; modspec.py) ----
MODSPEC_JMAX = 64                          # sa_modspec_dim(3)
MODSPEC_FRAME_RATE = 100.0                 # 16000 / 160 frames a second
MODSPEC_CUTOFF_LOW, MODSPEC_CUTOFF_HIGH = 3.2, 50.0      # J = ceil(200 / cutoff) stays under 64; 50 Hz is Nyquist

_ms_in = functools.partial(_aug_in, family="modulation-spectrum")
_modspec_taps = {}


def _modspec_half(cutoff_hz):
    """h[0..J] of modspec_taps as Python floats: a Hann-windowed sinc, the sine taken of the argument's distance to
    the nearest whole number so that a whole argument gives an exact zero (at 50 Hz the taps are the identity)"""
    J = math.ceil(200.0 / cutoff_hz)
    h = []
    for j in range(J + 1):
        x = 2.0 * cutoff_hz * j / MODSPEC_FRAME_RATE
        n = round(x)
        sinc = 1.0 if x == 0.0 else (-1.0 if n % 2 else 1.0) * math.sin(math.pi * (x - n)) / (math.pi * x)
        h.append(sinc * (0.5 + 0.5 * math.cos(math.pi * j / (J + 1))))
    total = h[0] + 2.0 * math.fsum(h[1:])
    return [v / total for v in h], J


def modspec_taps(cutoff_hz, device):
    """(taps fp64 [J + 1] on ``device``, J): the half h[0..J] of the symmetric low-pass along time at ``cutoff_hz`` of
    the 100 Hz frame rate, J = ceil(200 / cutoff_hz), h_j ~ sinc(2 cutoff j / 100) (0.5 + 0.5 cos(pi j / (J + 1))),
    normalised to h0 + 2 sum h_j = 1; built in fp64 on the host once per (cutoff, device)"""
    if isinstance(cutoff_hz, bool) or not MODSPEC_CUTOFF_LOW <= float(cutoff_hz) <= MODSPEC_CUTOFF_HIGH:
        raise L.SaHipError(f"modspec_taps: cutoff_hz {cutoff_hz} in {MODSPEC_CUTOFF_LOW:g}..{MODSPEC_CUTOFF_HIGH:g} "
                           "expected (the filter has at most 64 taps a side, and 50 Hz is the frame rate's Nyquist)")
    key = (float(cutoff_hz), torch.device(device))
    t = _modspec_taps.get(key)
    if t is None:
        h, _ = _modspec_half(key[0])
        t = _modspec_taps[key] = torch.tensor(h, dtype=torch.float64).to(key[1])
    return t, t.numel() - 1


def modspec_workspace(B, T, device):
    """the workspace sa_modspec_smooth takes (sa_modspec_workspace_bytes: the partial maxima of every row), as one
    8-byte-aligned buffer"""
    nbytes = L.load().sa_modspec_workspace_bytes(int(B), int(T))
    if nbytes < 0:
        raise L.SaHipError(f"modspec_workspace: [B, T] = [{B}, {T}] refused")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def modspec_smooth(R, taps, depth, frames, floor_rel=1e-4, max_gain_db=40.0, return_log=False):
    """R complex64 [B, T, 201], taps fp64 [J + 1] (the half of a symmetric FIR along time, J up to 64), depth fp32 [B]
    (taken into [0, 1], a NaN as 0), frames int32 [B] (clamped to [0, T]) -> (C complex64 [B, T, 201], peak fp64 [B]):
    C = R exp(g), g = clamp(depth (smoothed L - L), +-max_gain_db ln 10 / 20), L = ln max(|R|, floor_rel peak, 1e-10)
    with edge replication inside the row's frames; frames past them, and rows of depth 0, are R's bits
    (sa_modspec_smooth).  return_log: also L + g fp64 [B, T, 201], zero past the row's frames (tests)."""
    B, T = _gl_spec(R, "R", torch.complex64, _ms_in, 1)
    if _ms_in(taps, "taps", torch.float64).dim() != 1 or not 1 <= taps.numel() <= MODSPEC_JMAX + 1:
        raise L.SaHipError(f"taps: expected [J + 1] with J in 0..{MODSPEC_JMAX}, got {tuple(taps.shape)}")
    _ms_in(depth, "depth", shape=(B,))
    _ms_in(frames, "frames", torch.int32, (B,))
    if not 0.0 < float(floor_rel) < 1.0:
        raise L.SaHipError(f"modspec_smooth: floor_rel = {floor_rel} in (0, 1) expected")
    if not float(max_gain_db) > 0.0:
        raise L.SaHipError(f"modspec_smooth: max_gain_db = {max_gain_db} > 0 expected")
    out = torch.empty_like(R)
    peak = torch.empty(B, dtype=torch.float64, device=R.device)
    Lout = torch.empty(B, T, 201, dtype=torch.float64, device=R.device) if return_log else None
    ws = modspec_workspace(B, T, R.device)
    L.check(L.load().sa_modspec_smooth(_f(R), _f(taps), taps.numel() - 1, _f(depth), _f(frames), B, T,
                                       C.c_float(float(floor_rel)), C.c_float(float(max_gain_db) * LN10_OVER_20),
                                       _f(out), _f(peak), _f(Lout), _f(ws), L.stream()), "sa_modspec_smooth")
    return (out, peak, Lout) if return_log else (out, peak)


# ---- WSOLA time-scale modification (csrc/sa_wsola.hip; timescale.py) ----
WSOLA_H, WSOLA_W, WSOLA_D, WSOLA_Q = 160, 320, 160, 16383          # sa_wsola_dim(0..3)
WSOLA_MAX_N, WSOLA_MAX_NOUT = 1 << 24, 1 << 25
WSOLA_ONE = 1 << 16                        # tempo_q of tempo 1; the kernels take 2^15..2^17
WSOLA_QTILE = 4096                         # sa_wsola_dim(6): the samples per partial maximum

_wso_in = functools.partial(_aug_in, family="WSOLA")
_wsola_windows = {}


def _wso_dims(who, B, N, Nout=None):
    if not 1 <= B <= GL_MAX_B or not 1 <= N <= WSOLA_MAX_N:
        raise L.SaHipError(f"{who}: [B, N] = [{B}, {N}] -- B in 1..{GL_MAX_B} (a grid extent), N in 1..{WSOLA_MAX_N}")
    if Nout is not None and not 1 <= Nout <= WSOLA_MAX_NOUT:
        raise L.SaHipError(f"{who}: Nout = {Nout} in 1..{WSOLA_MAX_NOUT} expected")


def _wso_wav(who, wav, n_valid):
    if _wso_in(wav, "wav").dim() != 2 or wav.numel() == 0:
        raise L.SaHipError(f"wav: expected [B, N] with B, N >= 1, got {tuple(wav.shape)}")
    B, N = wav.shape
    _wso_in(n_valid, "n_valid", torch.int32, (B,))
    _wso_dims(who, B, N)
    return B, N


def wsola_out_len(n, tempo_q):
    """the samples a row of ``n`` valid ones has at ``tempo_q`` (units of 2^-16, read as 2^15..2^17): host integers,
    (n 2^16 + tempo_q / 2) / tempo_q, what sa_wsola_out_len returns -- the host sizes the output with it"""
    n, tq = int(n), min(max(int(tempo_q), WSOLA_ONE // 2), 2 * WSOLA_ONE)
    if not 0 <= n <= WSOLA_MAX_N:
        raise L.SaHipError(f"wsola_out_len: n = {n} in 0..{WSOLA_MAX_N} expected")
    return ((n << 16) + tq // 2) // tq if n else 0


def wsola_workspace_bytes(B, N):
    """sa_wsola_workspace_bytes as host integers: q, then the partial maxima, each rounded up to 16 bytes"""
    B, N = int(B), int(N)
    return ((2 * B * N + 15) & ~15) + ((4 * B * ((N + 3 + WSOLA_QTILE - 1) // WSOLA_QTILE) + 15) & ~15)


def wsola_workspace(B, N, device):
    """the workspace the WSOLA kernels share (sa_wsola_workspace_bytes), int16: q [B][N] at its start"""
    _wso_dims("wsola_workspace", int(B), int(N))
    return torch.empty(wsola_workspace_bytes(B, N) // 2, dtype=torch.int16, device=device)


def wsola_window(device):
    """hann fp32 [320] on ``device``: 0.5 - 0.5 cos(2 pi j / 320), formed in fp64 on the host and rounded once; built
    once per device"""
    key = torch.device(device)
    t = _wsola_windows.get(key)
    if t is None:
        h = [0.5 - 0.5 * math.cos(2.0 * math.pi * j / WSOLA_W) for j in range(WSOLA_W)]
        t = _wsola_windows[key] = torch.tensor(h, dtype=torch.float64).to(torch.float32).to(key)
    return t


def _wso_ws(ws, B, N):
    _wso_in(ws, "ws", torch.int16)
    if ws.dim() != 1 or ws.numel() * 2 < wsola_workspace_bytes(B, N) or ws.data_ptr() % 16:
        raise L.SaHipError(f"ws: expected wsola_workspace({B}, {N}), int16 [{wsola_workspace_bytes(B, N) // 2}], "
                           f"16-byte aligned; got {tuple(ws.shape)}")
    return ws


def wsola_quant(wav, n_valid, ws=None):
    """wav fp32 [B, N], n_valid int32 [B] -> q int16 [B, N], a view of the workspace's start: the search signal,
    rint(wav 16383 / peak) with the row's largest finite |wav| below n_valid as the peak, 0 where the sample is not
    finite or does not count (sa_wsola_quant).  ``ws``: a wsola_workspace to write into."""
    B, N = _wso_wav("wsola_quant", wav, n_valid)
    ws = wsola_workspace(B, N, wav.device) if ws is None else _wso_ws(ws, B, N)
    L.check(L.load().sa_wsola_quant(_f(wav), _f(n_valid), B, N, _f(ws), L.stream()), "sa_wsola_quant")
    return ws[:B * N].view(B, N)


def _wso_tempo(tempo_q, B):
    return _wso_in(tempo_q, "tempo_q", torch.int32, (B,))


def wsola_search(q, tempo_q, n_valid, Nout):
    """wsola_quant's q int16 [B, N], tempo_q int32 [B] (units of 2^-16, read as 2^15..2^17), n_valid int32 [B], Nout
    -> (pos int32 [B, (Nout - 1) // 160 + 1], count int32 [B], n_out int32 [B]): where every window of the output is
    cut from the input, how many there are and how many samples they give; entries of pos from count on mean nothing
    (sa_wsola_search)"""
    if _wso_in(q, "q", torch.int16).dim() != 2 or q.numel() == 0:
        raise L.SaHipError(f"q: expected [B, N] with B, N >= 1, got {tuple(q.shape)}")
    B, N = q.shape
    Nout = int(Nout)
    _wso_dims("wsola_search", B, N, Nout)
    if q.data_ptr() % 16:
        raise L.SaHipError("q: expected 16-byte aligned rows' start (wsola_quant's)")
    _wso_tempo(tempo_q, B)
    _wso_in(n_valid, "n_valid", torch.int32, (B,))
    pos = torch.empty(B, (Nout - 1) // WSOLA_H + 1, dtype=torch.int32, device=q.device)
    count, n_out = (torch.empty(B, dtype=torch.int32, device=q.device) for _ in range(2))
    L.check(L.load().sa_wsola_search(_f(q), _f(tempo_q), _f(n_valid), B, N, Nout, _f(pos), _f(count), _f(n_out),
                                     L.stream()), "sa_wsola_search")
    return pos, count, n_out


def wsola_ola(wav, pos, count, tempo_q, n_valid, Nout):
    """the overlap-add of wsola_search's windows: wav fp32 [B, N], pos, count, tempo_q, n_valid, Nout -> out fp32
    [B, Nout], zero from the row's n_out on; a stretch whose windows are contiguous in the input is a copy
    (sa_wsola_ola)"""
    B, N = _wso_wav("wsola_ola", wav, n_valid)
    Nout = int(Nout)
    _wso_dims("wsola_ola", B, N, Nout)
    _wso_in(pos, "pos", torch.int32, (B, (Nout - 1) // WSOLA_H + 1))
    _wso_in(count, "count", torch.int32, (B,))
    _wso_tempo(tempo_q, B)
    out = torch.empty(B, Nout, dtype=torch.float32, device=wav.device)
    L.check(L.load().sa_wsola_ola(_f(wav), _f(pos), _f(count), _f(tempo_q), _f(n_valid), _f(wsola_window(wav.device)),
                                  B, N, Nout, _f(out), L.stream()), "sa_wsola_ola")
    return out


def wsola(wav, tempo_q, n_valid, Nout, return_pos=False):
    """wav fp32 [B, N], tempo_q int32 [B], n_valid int32 [B], Nout -> (out fp32 [B, Nout], n_out int32 [B]): every row
    played at tempo_q / 2^16 of its speed, pitch and envelope kept, n_out = min(Nout, wsola_out_len(n_valid,
    tempo_q)) samples and zeros after them -- quantisation, search and overlap-add in one library call (sa_wsola),
    nothing copied to the host.  return_pos: also (pos, count)."""
    B, N = _wso_wav("wsola", wav, n_valid)
    Nout = int(Nout)
    _wso_dims("wsola", B, N, Nout)
    _wso_tempo(tempo_q, B)
    dev = wav.device
    ws = wsola_workspace(B, N, dev)
    out = torch.empty(B, Nout, dtype=torch.float32, device=dev)
    pos = torch.empty(B, (Nout - 1) // WSOLA_H + 1, dtype=torch.int32, device=dev)
    count, n_out = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    L.check(L.load().sa_wsola(_f(wav), _f(tempo_q), _f(n_valid), _f(wsola_window(dev)), B, N, Nout, _f(ws), _f(out),
                              _f(pos), _f(count), _f(n_out), L.stream()), "sa_wsola")
    return (out, n_out, pos, count) if return_pos else (out, n_out)
