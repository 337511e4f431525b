"""Inputs, conditions and references for the scoring stage beyond unit-variance inputs (test infrastructure, like decode_ref.py).

The scoring stage is the window QK^T, the fp32 softmax, the window sum, the pooling and the top-k.  synth.make_qkv keeps its
logits so narrow that the exponential's argument x - m never leaves [-12, 0], no row maximum is negative and no pooled score is
exactly 0.  The regimes below leave that range on purpose.  Each is built on synth.normal (portable, seeded) and is DEFINED by
conditions on the oracle's intermediates (`conditions`), not by its scale: a case that misses a condition gets another seed or
scale, never another condition.

  spread       q * s.  Every logit and pooled score finite (fp16: the mask may make -inf in the W x W corner); at least Hq * W
               arguments x - m in [-93, -86.6], the band where exp gives an fp32 subnormal; in every head n_keep makes the top-k
               take at least 8 exactly-zero pooled scores and leave at least 8 out (the tie order among +0.0, end to end).
  negative     q = |x| * s, k = -|x|.  Every row maximum is below -4: a maximum that started from 0 is wrong in every row.
  holes        every 5th key row and one window query row are all zero: exactly-zero logits inside tiles whose other logits are
               not (the out-of-guard arm of ScaleDiv<128> and tile_in_guard on a mixed tile).  Every scored row has at least
               floor((L - W) / 5) exactly-zero logits in the prefix columns.  (floor(L / 5) over all L columns cannot be had in
               the first window rows: the finfo.min triangle covers the corner's fifth columns.)
  edge_needle  keys equal to 4 x the mean window query (as synth's peaky does) planted at columns 0, 31, 32, L - W - 1, L - W and,
               5 x, at L - 1.  Each window row's maximum over its visible columns sits on a planted column; column L - 1 is
               visible to the last row only and carries the LARGEST needle, so a maximum that folds it into a row that cannot see
               it is wrong (six equal needles would leave that fault invisible).

References: softmax64 (fp64 softmax of given logits), torch_scores (the reference's arithmetic in live torch CPU operations) and
softmax_np (the softmax stage restated in numpy fp32, correct or with one of three faults, for the mutant test).
"""
import math
from collections import namedtuple

import numpy as np
import torch

from kvcache_factory_amd import synth

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
_DT_NAME = {BF16: "bf16", FP16: "fp16", FP32: "fp32"}

BAND_LO, BAND_HI = -93.0, -86.6          # arguments x - m whose exponential is an fp32 (and bf16) subnormal
ZERO_TIES = 8                            # spread: zeros the top-k must take, and leave, in every head


class Spec(namedtuple("Spec", "form regime dtype D Hq Hkv L W pooling kernel n_keep scale seed")):
    """form: snap (W = 8: softmax paths split / fused / fused_r2) | rows16 (W = 16 / 32 / 64: the same three paths; W = 32 also
    debug_mask 512) | h2o (fused, debug_mask 2048, 128 | 2048) | ragged (AdaKV, window MEAN) | cam | decode (split cache)."""
    __slots__ = ()

    @property
    def name(self):
        return (f"{self.form}-{self.regime}-{_DT_NAME[self.dtype]}-D{self.D}-H{self.Hq}x{self.Hkv}-L{self.L}-W{self.W}-"
                f"{self.pooling or 'none'}{self.kernel}-s{self.scale}")

    @property
    def full_rows(self):                 # the oracle's full_rows: 1 H2O (all L rows), 2 window mean, 0 window sum
        return {"h2o": 1, "ragged": 2}.get(self.form, 0)


def _s(form, regime, dtype, D, Hq, Hkv, L, W, pooling, kernel, n_keep, scale, seed):
    return Spec(form, regime, dtype, D, Hq, Hkv, L, W, pooling, kernel, n_keep, scale, seed)


# Shapes: the smallest at which each form can still go wrong — L = 300 / 97 / 264 (one ragged tile, L % 8 != 0, L % 16 == 8),
# L = 1100 / 1304 (several tiles, a ragged last one, the chain / worker kernel from L = 1024), both head dims, GQA and not.
# spread's n_keep: max over heads of the non-zero pooled scores + ZERO_TIES (test_score_range_cpu.py checks the condition).
# spread's scale: 160 (bf16 / fp32) leaves fewer than Hq * W arguments in the band at L = 300; 100 meets every condition.
GRID = [
    # ---- SnapKV, W = 8 ------------------------------------------------------------------------------------------------------
    _s("snap", "spread", BF16, 128, 4, 2, 300, 8, "maxpool", 7, 272, 100, 11),
    _s("snap", "spread", BF16, 64, 4, 2, 1100, 8, "avgpool", 5, 532, 100, 12),
    _s("snap", "spread", FP16, 128, 4, 2, 1100, 8, "maxpool", 7, 230, 40, 13),
    _s("snap", "spread", FP16, 64, 4, 2, 300, 8, "avgpool", 5, 120, 40, 14),
    _s("snap", "spread", FP32, 128, 4, 2, 300, 8, "avgpool", 5, 262, 100, 15),
    _s("snap", "spread", FP32, 64, 4, 2, 1100, 8, "maxpool", 7, 806, 100, 16),
    _s("snap", "spread", BF16, 128, 2, 2, 8200, 8, "maxpool", 7, 664, 160, 17),        # exponentials recomputed beyond 8k keys
    _s("snap", "negative", BF16, 128, 4, 2, 1100, 8, "maxpool", 7, 64, 1, 21),
    _s("snap", "negative", FP16, 128, 4, 2, 300, 8, "avgpool", 5, 64, 1, 22),
    _s("snap", "negative", FP32, 64, 4, 2, 300, 8, "maxpool", 7, 64, 8, 23),
    _s("snap", "negative", BF16, 64, 4, 2, 300, 8, "avgpool", 5, 64, 8, 24),
    _s("snap", "negative", BF16, 128, 4, 2, 300, 8, "maxpool", 7, 64, 32, 25),          # maxima near -230: see softmax_np
    _s("snap", "holes", BF16, 64, 4, 2, 300, 8, "maxpool", 7, 64, 1, 31),
    _s("snap", "holes", FP16, 128, 4, 2, 1100, 8, "avgpool", 5, 64, 1, 32),
    _s("snap", "holes", FP32, 128, 4, 2, 1100, 8, "maxpool", 7, 64, 1, 33),
    _s("snap", "edge_needle", BF16, 128, 2, 2, 300, 8, "avgpool", 5, 64, 10, 41),
    _s("snap", "edge_needle", FP16, 128, 2, 2, 1100, 8, "maxpool", 7, 64, 2, 42),
    _s("snap", "edge_needle", FP32, 128, 2, 2, 300, 8, "maxpool", 7, 64, 10, 43),
    _s("snap", "edge_needle", BF16, 64, 2, 2, 1100, 8, "maxpool", 7, 64, 4, 44),
    # ---- W = 16 / 32 / 64: 16 rows per workgroup, logits_mt4_kernel where G * W == 128 ---------------------------------------
    _s("rows16", "spread", BF16, 128, 8, 2, 1100, 16, "maxpool", 7, 945, 100, 51),
    _s("rows16", "spread", FP16, 128, 8, 2, 1100, 32, "avgpool", 5, 461, 40, 52),       # G * W == 128: four M tiles per K tile
    _s("rows16", "negative", BF16, 64, 4, 2, 1100, 64, "maxpool", 7, 64, 8, 53),        # G * W == 128
    _s("rows16", "holes", BF16, 128, 4, 2, 97, 32, "maxpool", 7, 30, 1, 54),
    _s("rows16", "negative", FP16, 64, 4, 2, 97, 16, "avgpool", 5, 30, 8, 55),
    _s("rows16", "negative", BF16, 128, 4, 2, 1100, 32, "maxpool", 7, 64, 1, 56),        # G * W != 128
    _s("rows16", "holes", BF16, 128, 8, 2, 1100, 16, "avgpool", 5, 64, 1, 57),           # G * W == 128
    _s("rows16", "holes", FP16, 64, 4, 2, 97, 64, "maxpool", 7, 20, 1, 58),
    # ---- H2O: all L rows; L % 8 == 0 the wide form (264: L % 16 == 8), else the one-column form --------------------------------
    _s("h2o", "spread", BF16, 128, 4, 2, 300, 8, None, 7, 249, 400, 61),
    _s("h2o", "spread", BF16, 64, 4, 2, 264, 8, None, 7, 214, 400, 62),
    _s("h2o", "spread", FP16, 128, 4, 2, 300, 8, None, 7, 282, 40, 63),
    _s("h2o", "negative", BF16, 128, 4, 2, 1304, 8, None, 7, 64, 8, 64),
    _s("h2o", "negative", FP16, 64, 4, 2, 264, 8, None, 7, 64, 8, 65),
    _s("h2o", "holes", FP16, 128, 4, 2, 300, 8, None, 7, 64, 1, 66),
    _s("h2o", "holes", FP32, 64, 2, 2, 264, 8, None, 7, 64, 1, 67),
    _s("h2o", "edge_needle", BF16, 128, 2, 2, 264, 8, None, 7, 64, 2, 68),
    # ---- the ragged window mean (AdaKV), CAM, and the split decode cache ------------------------------------------------------
    _s("ragged", "spread", BF16, 128, 4, 2, 300, 8, "maxpool", 7, 271, 100, 71),
    _s("ragged", "negative", FP16, 128, 4, 2, 300, 8, "maxpool", 7, 64, 1, 72),
    _s("cam", "spread", BF16, 128, 4, 2, 300, 8, "maxpool", 1, 93, 100, 73),
    _s("cam", "negative", FP32, 64, 4, 2, 300, 8, "maxpool", 1, 64, 8, 74),
    _s("decode", "spread", BF16, 128, 4, 2, 300, 8, "maxpool", 7, 276, 100, 75),        # prefix 200 rows, tail 100
]
DECODE_PREFIX = 200
NEEDLE_ROW = 3                            # holes: the all-zero window query row


def needle_columns(spec):
    L, W = spec.L, spec.W
    return [0, 31, 32, L - W - 1, L - W, L - 1]


def inputs(spec):
    """(q [1, Hq, L, D] in the model's memory order, k, v [1, Hkv, L, D]) of a spec, on the CPU."""
    Hq, Hkv, L, D, W, dt = spec.Hq, spec.Hkv, spec.L, spec.D, spec.W, spec.dtype
    q = synth.normal((1, L, Hq, D), spec.seed, 0)
    k = synth.normal((1, Hkv, L, D), spec.seed, 1)
    v = synth.normal((1, Hkv, L, D), spec.seed, 2).to(dt)
    if spec.regime == "negative":
        q, k = q.abs() * float(spec.scale), -k.abs()
    else:
        q = q * float(spec.scale)
    if spec.regime == "holes":
        k[:, :, ::5] = 0.0
        q[:, L - W + NEEDLE_ROW] = 0.0
    if spec.regime == "edge_needle":
        g = Hq // Hkv
        for h in range(Hkv):
            qbar = q[0, L - W:, h * g].to(dt).float().mean(0)
            k[0, h, needle_columns(spec)] = 4.0 * qbar
            k[0, h, L - 1] = 5.0 * qbar
    return q.to(dt).transpose(1, 2), k.to(dt), v


# ---- conditions -----------------------------------------------------------------------------------------------------------------
def visible(spec, R):
    """bool [R, L]: the columns a scored row sees (everything but the strict upper triangle of the W x W corner)."""
    L, W = spec.L, spec.W
    vis = torch.ones(R, L, dtype=torch.bool)
    vis[R - W:, L - W:] = torch.ones(W, W, dtype=torch.bool).tril()
    return vis


def conditions(spec, lg, sc):
    """Check the regime's conditions on the oracle's logits lg [H, R, L] and pooled scores sc [H, n]; return the counts."""
    L, W = spec.L, spec.W
    x = lg.float()
    R = x.shape[1]
    vis = visible(spec, R)
    m = x.max(-1, keepdim=True).values
    arg = x - m
    out = {"rowmax_min": float(m.min()), "rowmax_max": float(m.max())}
    assert not torch.isnan(x).any() and not torch.isnan(sc.float()).any()
    assert torch.isfinite(x[:, vis]).all() and torch.isfinite(sc.float()).all() and torch.isfinite(m).all()
    if spec.dtype != FP16:
        assert torch.isfinite(x).all()                       # only fp16's finfo.min can round a masked logit to -inf
    if spec.regime == "spread":
        band = int(((arg >= BAND_LO) & (arg <= BAND_HI)).sum())
        zeros = (sc.float() == 0).sum(-1)
        n = sc.shape[1]
        keep = spec.n_keep
        taken = keep - (n - zeros)                           # zeros the top-k must take, per head
        out.update(band=band, zeros_min=int(zeros.min()), zeros_max=int(zeros.max()), n_keep=keep,
                   zeros_taken_min=int(taken.min()), zeros_left_min=int((zeros - taken).min()))
        assert band >= spec.Hq * W, out
        assert int(taken.min()) >= ZERO_TIES and int((zeros - taken).min()) >= ZERO_TIES, out
    elif spec.regime == "negative":
        assert float(m.max()) < -4.0, out
    elif spec.regime == "holes":
        z = (x[:, :, :L - W] == 0).sum(-1)
        out.update(zero_logits_min=int(z.min()), zero_logits_max=int(z.max()))
        assert int(z.min()) >= (L - W) // 5, out
        assert int(z[:, R - W + NEEDLE_ROW].min()) == L - W                        # the zero query row: every logit is 0
        live = torch.ones(R, dtype=torch.bool)
        live[R - W + NEEDLE_ROW] = False
        assert int(z[:, live].max()) < (L - W) // 4, out                             # ... and elsewhere the tiles are mixed
    elif spec.regime == "edge_needle":
        cols = needle_columns(spec)
        xw, vw = x[:, R - W:], vis[R - W:]
        mv = xw.masked_fill(~vw, float("-inf")).max(-1).values                      # maximum over the visible columns [H, W]
        planted = xw[:, :, cols].masked_fill(~vw[:, cols], float("-inf")).max(-1).values
        assert torch.equal(mv, planted), out
        assert vw[:, L - 1].sum() == 1 and bool(vw[W - 1, L - 1])
        hidden = xw[:, :W - 1, L - 1]                                                # masked: finfo.min was added
        out.update(needle_logit_min=float(mv.min()), masked_last_col_max=float(hidden.max()))
        assert float(hidden.max()) < -1e4
    return out


# ---- references -----------------------------------------------------------------------------------------------------------------
def softmax64(lg):
    """fp64 softmax over the last dimension of logits given in any dtype (-inf allowed, not a whole row of it)."""
    return torch.softmax(lg.double(), -1)


def ulp_of(p64, dtype):
    """Spacing of `dtype` at the magnitude of the fp64 values p64 (the subnormal spacing below the smallest normal)."""
    mant, emin = {BF16: (7, -126), FP16: (10, -14), FP32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(p64.clamp(min=2.0 ** -300))).clamp(min=emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def prob_bound(p64, dtype):
    """|p - p64| <= 1/2 ulp_dtype(p64) + 2^-17 p64 + 2^-149.  2^-17 is derived, not fitted: half an fp32 unit of an argument below
    128 is 2^-18 (the relative error it causes in exp), the degree-5 polynomial adds about 2^-20, the reciprocal, the sum and the
    product a few 2^-24; 2^-149 is one unit of the subnormal the exponential rounds into; the first term is the rounding to dtype."""
    return 0.5 * ulp_of(p64, dtype) + 2.0 ** -17 * p64 + 2.0 ** -149


def torch_scores(spec, q, k):
    """The reference's arithmetic in live torch CPU operations: matmul / sqrt(D), the finfo.min triangle added in dtype,
    softmax(dtype=float32).to(dtype), the window sum (H2O: the sum over all rows; ragged: the window mean), max_pool1d /
    avg_pool1d.  Returns pooled scores [Hq, n]."""
    W, D, dt = spec.W, spec.D, spec.dtype
    kx = k.repeat_interleave(spec.Hq // spec.Hkv, 1)
    rows = q if spec.form == "h2o" else q[:, :, -W:]
    a = torch.matmul(rows, kx.transpose(2, 3)) / math.sqrt(D)
    a[:, :, -W:, -W:] += torch.full((W, W), torch.finfo(dt).min, dtype=dt).triu(1)
    p = torch.softmax(a, -1, dtype=torch.float32).to(dt)
    s = p[:, :, :, :-W].mean(-2) if spec.form == "ragged" else p[:, :, :, :-W].sum(-2)
    if spec.form != "h2o":
        pool = torch.nn.functional.max_pool1d if spec.pooling == "maxpool" else torch.nn.functional.avg_pool1d
        s = pool(s, kernel_size=spec.kernel, padding=spec.kernel // 2, stride=1)
    return s[0]


def oracle_scores(oracle, spec, q, k, want_intermediates=False):
    """The oracle in product mode on a spec."""
    return oracle.scores(q, k, spec.W, spec.kernel, spec.pooling or "avgpool", full_rows=spec.full_rows,
                         want_intermediates=want_intermediates, dot_mode=oracle.DOT_CHAIN, sum_mode=oracle.SUM_TORCH16)


def oracle_rowmax_rowsum(oracle, lg):
    """The fp32 row maxima and softmax denominators [H, R] the oracle's softmax forms from its logits lg [H, R, L]: the maximum over
    all L columns, and the sum of exp_u20(x - m) in torch's 16-lane order — what the kernels leave in the workspace."""
    import ctypes
    x = lg.float()
    m = x.max(-1).values
    e = oracle.exp_u20((x - m[..., None]).contiguous())
    rows = e.view(-1, e.shape[-1])
    s = torch.tensor([oracle.lib().kvco_sum(ctypes.c_void_p(r.data_ptr()), r.numel(), oracle.SUM_TORCH16) for r in rows],
                     dtype=torch.float32)
    return m, s.view(m.shape)


FAULTS = ("max_from_zero", "folded_column", "flush_below_87")


def softmax_np(lg, dtype, fault=None, hidden=None):
    """The softmax stage in numpy fp32 on logits lg [H, R, L] (the last W rows are the window): m = max, e = exp(x - m) rounded to
    fp32, s = sum, p = e * (1 / s), rounded to dtype.  fault: None, or one of FAULTS —
      max_from_zero    the running maximum starts from 0 instead of the first logit;
      folded_column    the rows that cannot see column L - 1 fold `hidden` [H, W - 1], its unmasked logit, into their maximum;
      flush_below_87   the exponential's lower clamp sits at -87.0 and gives +0 there, as the header's 2^(n-1) does.
    A shifted maximum leaves a softmax unchanged until exponentials underflow, so the first two faults show in the probabilities
    only where the shift is large: row maxima near -230 (negative, s = 32), needles near +500 whose 5 x twin is 125 above them
    (edge_needle, s = 10).  Smaller shifts show in the row maxima, which the GPU test compares bit for bit."""
    x = lg.float().numpy().astype(np.float32)
    m = x.max(-1)
    if fault == "max_from_zero":
        m = np.maximum(m, np.float32(0))
    if fault == "folded_column":
        W1 = hidden.shape[1]
        m[:, -W1 - 1:-1] = np.maximum(m[:, -W1 - 1:-1], hidden.float().numpy())
    arg = (x - m[..., None]).astype(np.float32)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(arg.astype(np.float64)).astype(np.float32)
        if fault == "flush_below_87":
            e = np.where(arg <= np.float32(-87.0), np.float32(0), e)
        s = e.sum(-1, dtype=np.float32)
        p = (e * (np.float32(1) / s)[..., None]).astype(np.float32)
    return torch.from_numpy(p).to(dtype)


def hidden_last_column(spec, q, k):
    """The logit of column L - 1 WITHOUT the mask for the window rows that cannot see it [Hq, W - 1], rounded like a logit."""
    W, dt = spec.W, spec.dtype
    kx = k.repeat_interleave(spec.Hq // spec.Hkv, 1)
    d = (q[0, :, -W:-1].double() * kx[0, :, -1:].double()).sum(-1).float().to(dt).float()
    return (d / math.sqrt(spec.D)).to(dt)


def probs_within_bound(p, lg, dtype):
    """(ok, worst): every probability p (dtype) within prob_bound of softmax64(lg); worst = max of |p - p64| / bound (nan = inf)."""
    p64 = softmax64(lg)
    ratio = (p.double() - p64).abs() / prob_bound(p64, dtype)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return bool((ratio <= 1.0).all()), float(ratio.max())


def rel_excess(p, lg, dtype):
    """max over elements of (|p - p64| - 1/2 ulp - 2^-149) / p64: the part of the error the 2^-17 term has to cover."""
    p64 = softmax64(lg)
    ex = ((p.double() - p64).abs() - 0.5 * ulp_of(p64, dtype) - 2.0 ** -149) / p64.clamp(min=2.0 ** -1000)
    return float(ex[p64 > 0].max())
