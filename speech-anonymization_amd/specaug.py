"""SpecAugment of the input features in the ConvAE train step: the reference's
``hparams.augmentation`` (speechbrain_convae_train.py:65-67, convae.yaml:273-283), restated from speechbrain 0.5.x
lobes/augment.py::SpecAugment -- parity with its device-side random stream unpinned -- and run as three launches of
csrc/sa_specaug.hip: time warp + sums, the two fill values, the masks.

Every draw is made on the host from a ``torch.Generator`` the module owns and travels to the device as one PLAN of
32-bit words, copied asynchronously from pinned memory into a buffer the module keeps per (B, T, F), so that the
launches depend on (B, T, F) alone and can sit in a captured graph.  Nothing here reads device memory or
synchronises.

Plan words: header [8] (flags, B, T, F, 0 ...) | rows [T][8] (base, lo, hi, 0 as int; four weights as float:
output row o = sum_k w[k] x[clamp(base - 1 + k, lo, hi)]) | freq [B][8][2] (pos, len) | time [B][8][2] |
n_fm [B] (frequency-masked cells of the utterance).
"""
import types

import torch

from . import _lib as L

HEADER = 8
ROW_WORDS = 8
MAX_MASKS = 8
MAX_F = 128
FLAG_ZERO = 1
A = -0.75

DEFAULTS = dict(time_warp=True, time_warp_window=5, time_warp_mode="bicubic", freq_mask=True,
                freq_mask_width=(0, 20), n_freq_mask=2, time_mask=True, time_mask_width=(0, 100), n_time_mask=2,
                replace_with_zero=True)


def _width(v, what):
    lo, hi = (0, v) if isinstance(v, int) else tuple(v)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi <= lo:
        raise ValueError(f"SpecAugment: {what} {v!r} -- a width is an int > 0 or a range (lo, hi) with 0 <= lo < hi")
    return lo, hi


def settings(cfg=None, **over):
    """DEFAULTS overlaid with a mapping (the YAML block), a settings object or keywords; checked"""
    out = dict(DEFAULTS)
    if cfg is not None:
        src = cfg if isinstance(cfg, dict) else vars(cfg)
        unknown = [k for k in src if k not in DEFAULTS]
        if unknown:
            raise ValueError(f"SpecAugment: unknown setting {unknown[0]!r}")
        out.update(src)
    out.update(over)
    c = types.SimpleNamespace(**out)
    if c.time_warp_mode != "bicubic":
        raise ValueError(f"SpecAugment: time_warp_mode {c.time_warp_mode!r} -- only bicubic is built")
    c.time_warp_window = int(c.time_warp_window)
    if c.time_warp_window < 1:
        raise ValueError("SpecAugment: time_warp_window must be at least 1")
    c.freq_mask_width = _width(c.freq_mask_width, "freq_mask_width")
    c.time_mask_width = _width(c.time_mask_width, "time_mask_width")
    for k in ("n_freq_mask", "n_time_mask"):
        n = int(getattr(c, k))
        if n < 0 or n > MAX_MASKS:
            raise ValueError(f"SpecAugment: {k} {n} -- a plan carries 0 to {MAX_MASKS} masks per axis")
        setattr(c, k, n)
    return c


def check_shape(B, T, F):
    if B < 1 or T < 1:
        raise ValueError(f"SpecAugment: features [{B}, {T}, {F}] -- B and T must be at least 1")
    if F < 4 or F % 4 or F > MAX_F:
        raise ValueError(f"SpecAugment: F = {F} -- the kernels take a multiple of 4 up to {MAX_F}")


def plan_words(B, T):
    """32-bit words of a plan for B utterances of T frames"""
    return HEADER + ROW_WORDS * T + (4 * MAX_MASKS + 1) * B


# ---- the table (fp32, as torch forms it) -------------------------------------------------------------------
def bicubic_table(n_in, n_out):
    """bicubic, align_corners=True, n_in -> n_out rows: (base int32 [n_out], w fp32 [n_out, 4]); output row o =
    sum_k w[o][k] x[clamp(base[o] - 1 + k, 0, n_in - 1)].  Index and coefficients in fp32, operation by operation
    as torch's upsample_bicubic2d forms them (A = -0.75)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"bicubic_table: {n_in} -> {n_out} rows")
    f32 = torch.float32
    scale = (torch.tensor(float(n_in - 1), dtype=f32) / torch.tensor(float(n_out - 1), dtype=f32)
             if n_out > 1 else torch.zeros((), dtype=f32))
    real = scale * torch.arange(n_out, dtype=f32)
    base = torch.floor(real).clamp(max=float(n_in - 1))
    t = (real - base).clamp(0.0, 1.0)
    a = torch.tensor(A, dtype=f32)

    def inner(u):          # |u| <= 1
        return ((a + 2.0) * u - (a + 3.0)) * u * u + 1.0

    def outer(u):          # 1 < |u| < 2
        return ((a * u - 5.0 * a) * u + 8.0 * a) * u - 4.0 * a

    s = 1.0 - t
    w = torch.stack([outer(t + 1.0), inner(t), inner(s), outer(s + 1.0)], 1)
    return base.to(torch.int32), w.to(f32).contiguous()


# ---- the plan ----------------------------------------------------------------------------------------------
class Plan:
    """one step's draws and tables.  B, T, F; c, w (None: the warp is the identity); base, lo, hi (int32 [T]) and
    wt (fp32 [T, 4]) per output row; freq, time: B lists of (pos, len); zero: replace_with_zero."""

    def masks(self):
        """(fm [B, F] bool, tm [B, T] bool)"""
        fm = torch.zeros(self.B, self.F, dtype=torch.bool)
        tm = torch.zeros(self.B, self.T, dtype=torch.bool)
        for m, rows, D in ((fm, self.freq, self.F), (tm, self.time, self.T)):
            for b, pairs in enumerate(rows):
                for pos, n in pairs:
                    m[b, max(pos, 0):max(min(pos + n, D), 0)] = True
        return fm, tm

    def words(self):
        """the plan buffer (int32, pinned where a GPU is present), laid out as the module docstring says"""
        head = torch.zeros(HEADER, dtype=torch.int32)
        head[0], head[1], head[2], head[3] = (FLAG_ZERO if self.zero else 0), self.B, self.T, self.F
        rows = torch.zeros(self.T, ROW_WORDS, dtype=torch.int32)
        rows[:, 0], rows[:, 1], rows[:, 2] = self.base, self.lo, self.hi
        rows[:, 4:] = self.wt.view(torch.int32)
        pairs = torch.zeros(2, self.B, MAX_MASKS, 2, dtype=torch.int32)
        for a, lists in enumerate((self.freq, self.time)):
            for b, lst in enumerate(lists):
                if len(lst) > MAX_MASKS:
                    raise ValueError(f"SpecAugment: a plan carries at most {MAX_MASKS} masks per axis, utterance {b} "
                                     f"has {len(lst)}")
                if lst:
                    pairs[a, b, :len(lst)] = torch.tensor(lst, dtype=torch.int32)
        n_fm = (self.masks()[0].sum(1) * self.T).to(torch.int32)
        parts = [head, rows.reshape(-1), pairs.reshape(-1), n_fm]
        buf = torch.empty(plan_words(self.B, self.T), dtype=torch.int32, pin_memory=torch.cuda.is_available())
        torch.cat(parts, out=buf)
        return buf


def make_plan(B, T, F, c=None, w=None, freq=(), time=(), cfg=None):
    """a plan from given draws (tests build edge cases with it; draw_plan draws and calls it).  c, w: the warp
    centre and its new position (both None: no warp); freq, time: B lists of (pos, len), or () for none."""
    cf = cfg if isinstance(cfg, types.SimpleNamespace) and hasattr(cfg, "n_time_mask") else settings(cfg)
    B, T, F = int(B), int(T), int(F)
    check_shape(B, T, F)
    p = Plan()
    p.B, p.T, p.F, p.zero = B, T, F, bool(cf.replace_with_zero)
    p.c, p.w = (None, None) if c is None else (int(c), int(w))
    ar = torch.arange(T, dtype=torch.int32)
    if p.c is None:
        p.base, p.lo, p.hi = ar.clone(), torch.zeros_like(ar), torch.full_like(ar, T - 1)
        p.wt = torch.tensor([0.0, 1.0, 0.0, 0.0]).repeat(T, 1)
    else:
        if not (1 <= p.c <= T - 1 and 1 <= p.w <= T - 1):
            raise ValueError(f"SpecAugment: warp c = {p.c}, w = {p.w} -- both segments need a row (T = {T})")
        lb, lw = bicubic_table(p.c, p.w)
        rb, rw = bicubic_table(T - p.c, T - p.w)
        p.base = torch.cat([lb, rb + p.c])
        p.lo = torch.cat([torch.zeros(p.w, dtype=torch.int32), torch.full((T - p.w,), p.c, dtype=torch.int32)])
        p.hi = torch.cat([torch.full((p.w,), p.c - 1, dtype=torch.int32),
                          torch.full((T - p.w,), T - 1, dtype=torch.int32)])
        p.wt = torch.cat([lw, rw])
    for name, lists in (("freq", freq), ("time", time)):
        lists = [[] for _ in range(B)] if len(lists) == 0 else [[(int(a), int(n)) for a, n in row] for row in lists]
        if len(lists) != B:
            raise ValueError(f"SpecAugment: {name}: one list of (pos, len) per utterance ({B}), got {len(lists)}")
        if any(a < 0 or n < 0 for row in lists for a, n in row):
            raise ValueError(f"SpecAugment: {name}: positions and lengths must not be negative")
        setattr(p, name, lists)
    return p


def _draw_masks(gen, B, D, width, n):
    if n == 0:
        return ()
    ln = torch.randint(width[0], width[1], (B, n), generator=gen)
    pos = torch.randint(0, max(1, D - int(ln.max())), (B, n), generator=gen)
    return [list(zip(pos[b].tolist(), ln[b].tolist())) for b in range(B)]


def draw_plan(gen, B, T, F, cfg=None):
    """one step's plan from the host generator ``gen``.  Draw order: c, w, frequency lengths, frequency positions,
    time lengths, time positions (upper bounds exclusive, as torch.randint's)."""
    cf = cfg if isinstance(cfg, types.SimpleNamespace) and hasattr(cfg, "n_time_mask") else settings(cfg)
    c = w = None
    win = cf.time_warp_window
    if cf.time_warp and T - win > win:
        c = int(torch.randint(win, T - win, (1,), generator=gen))
        w = int(torch.randint(c - win, c + win, (1,), generator=gen)) + 1
    freq = _draw_masks(gen, B, F, cf.freq_mask_width, cf.n_freq_mask) if cf.freq_mask else ()
    time = _draw_masks(gen, B, T, cf.time_mask_width, cf.n_time_mask) if cf.time_mask else ()
    return make_plan(B, T, F, c, w, freq, time, cf)


# ---- launches ----------------------------------------------------------------------------------------------
def apply_words(x, words):
    """x [B, T, F] (device, fp32, contiguous) and the device copy of a plan's words -> the augmented features, a
    new tensor: sa_specaug_warp_sums, sa_specaug_finalize, sa_specaug_fill"""
    from . import ops
    out, part = ops.specaug_warp_sums(x, words)
    vals = ops.specaug_finalize(part, words, *x.shape)
    return ops.specaug_fill(out, words, vals)


def apply_plan(x, plan):
    """one asynchronous copy of the plan, then the three launches"""
    _check_input(x)
    if tuple(x.shape) != (plan.B, plan.T, plan.F):
        raise ValueError(f"SpecAugment: the plan was drawn for [{plan.B}, {plan.T}, {plan.F}], got {tuple(x.shape)}")
    return apply_words(x, plan.words().to(x.device, non_blocking=True))


def _check_input(x):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("SpecAugment runs on the GPU only (no CPU fallback)")
    if x.dtype != torch.float32:
        raise ValueError(f"SpecAugment: expected float32 features, got {x.dtype}")
    if x.dim() != 3:
        raise ValueError(f"SpecAugment: expected features [B, T, F], got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("SpecAugment: expected contiguous features")
    check_shape(*x.shape)


class SpecAugment(torch.nn.Module):
    """speechbrain.lobes.augment.SpecAugment's constructor and defaults; ``(feats) -> feats'`` [B, T, F], a new
    tensor (the input is never written).  ``draw(B, T, F)`` draws the step's plan and copies it into the module's
    device buffer for that shape; ``apply(x)`` only launches on it (what a captured step records); calling the
    module does both.  ``reseed(epoch, rank)`` -- the brain calls it at every TRAIN stage start -- reseeds the
    generator from (seed, epoch, rank).  ``debug``: keep references to the last input and output (tests)."""

    def __init__(self, time_warp=True, time_warp_window=5, time_warp_mode="bicubic", freq_mask=True,
                 freq_mask_width=(0, 20), n_freq_mask=2, time_mask=True, time_mask_width=(0, 100), n_time_mask=2,
                 replace_with_zero=True, seed=1986):
        super().__init__()
        self.cfg = settings(time_warp=time_warp, time_warp_window=time_warp_window, time_warp_mode=time_warp_mode,
                            freq_mask=freq_mask, freq_mask_width=freq_mask_width, n_freq_mask=n_freq_mask,
                            time_mask=time_mask, time_mask_width=time_mask_width, n_time_mask=n_time_mask,
                            replace_with_zero=replace_with_zero)
        self.seed = int(seed)
        self.gen = torch.Generator()
        self.last_plan = self.last_input = self.last_output = None
        self.debug = False
        self._words = {}                  # (device, B, T, F) -> the persistent device copy of the plan
        self.reseed(0)

    def describe(self):
        c = self.cfg
        return (f"time warp {'window %d' % c.time_warp_window if c.time_warp else 'off'}, "
                f"{c.n_freq_mask if c.freq_mask else 0} frequency masks under {c.freq_mask_width[1]} bins, "
                f"{c.n_time_mask if c.time_mask else 0} time masks under {c.time_mask_width[1]} frames, filled with "
                f"{'zero' if c.replace_with_zero else 'the mean'}, seed {self.seed}")

    def reseed(self, epoch, rank=0):
        self.gen.manual_seed((self.seed * 100003 + int(epoch or 0)) * 4099 + int(rank))

    def draw(self, B, T, F, device=None):
        """draw the plan of one step for features [B, T, F] and send it to the device (one asynchronous copy)"""
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        plan = self.last_plan = draw_plan(self.gen, B, T, F, self.cfg)
        key = (device, plan.B, plan.T, plan.F)
        dev = self._words.get(key)
        if dev is None:
            dev = self._words[key] = torch.empty(plan_words(plan.B, plan.T), dtype=torch.int32, device=device)
        dev.copy_(plan.words(), non_blocking=True)
        return plan

    def apply(self, x):
        """the three launches on the plan last drawn for x's shape"""
        _check_input(x)
        dev = self._words.get((x.device, *x.shape))
        if dev is None:
            raise ValueError(f"SpecAugment.apply: no plan was drawn for features {tuple(x.shape)} on {x.device}")
        out = apply_words(x, dev)
        if self.debug:
            self.last_input, self.last_output = x, out
        return out

    def forward(self, x):
        _check_input(x)
        self.draw(*x.shape, device=x.device)
        return self.apply(x)
