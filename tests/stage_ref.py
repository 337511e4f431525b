"""Inputs, conditions and references for the stages that follow scoring and change the cache contents — the pivot merge
(kvc_merge.hip), ThinK channel pruning (kvc_think.hip), L2Norm (kvc_l2norm.hip) and the CAM value recurrence (kvc_cam.hip) —
beyond unit-variance keys (test infrastructure, like score_ref.py and decode_ref.py).

Every other test of these stages feeds synth.make_qkv or coarsened randn: a kept row of the merge then receives a few dozen
merges (its count never rounds in the dtype), two kept rows almost never share a rounded cosine, and no norm or channel score is
0, inf, NaN or built from fp32 subnormals.  The regimes below leave that range on purpose.  Each is built on synth.normal
(portable, seeded) and is DEFINED by conditions on the reference outputs (`conditions`), not by its scale: a spec that misses a
condition is an input error (AssertionError, never a skip) and gets another seed or size, never another condition.

  clustered         keys c + 0.3 n around one direction c per KV head, V x 8, n_keep 1-3; the window rows and all kept rows but one
                    per head are planted at -c + 0.3 n.  In every head one kept row receives a count c with dtype(c) != c (>= 257
                    and odd in bf16, >= 2049 and odd in fp16) and at least one 64-pivot chunk holds 64 equal pivots (a full ballot
                    of merge_reduce_kernel's walk).
  outlier_channels  two key channels offset by +40 and -25 (the keys real models produce: every cosine is near 1 and the rounded
                    cosines tie by the dozen), V x 30.
  duplicates        dropped and kept rows that are exact copies of three prototype rows per KV head, planted so that per head at
                    least 32 dropped tokens attain their maximal rounded cosine at kept rows in two different 64-row LDS stages, 32
                    in two different 32-row M-tiles of one stage, and 32 at rows r and r + 4 of one 8-row block (the two
                    half-waves); n_keep + W = 144.  The prototypes are the smallest rows, so the L2Norm cut falls inside a group of
                    equal norms in every head.
  overflow          fp16 only: keys x 3000 (every 5th row x 12 000: x 3000 alone leaves every norm near 34 000, finite), queries x 300,
                    V x 10 000, every third key channel zero.  Infinite norms exist; every ThinK channel score is inf or NaN (inf * 0) and
                    the two specs put the n_prune boundary among the infs and among the NaNs; the merged K' holds inf, and so do the values
                    CAM's recurrence leaves under an all-ones mask.
  zero_rows         every 7th key row is zero, among the dropped and among the kept rows (0 / 0 = NaN cosines).  Per head at least
                    one dropped token has only NaN cosines and at least one has NaN columns that are a proper subset with a finite
                    maximum elsewhere.  L = 700 puts zero row 693 into window column 1: every pivot of those two specs is 0 or 1, found
                    by the first lanes of the first tile.  A zero kept row is a WHOLE NaN column (a finite unit row times a NaN one), so
                    within a head every partly-NaN token has the same first NaN column, and it can vary only between heads.  The
                    `planted` variant (n_keep + W = 144, no zero row in the window, every selected row non-zero except the planted
                    slots) therefore gives each of its four heads another first NaN column: head 0 kept rows 12 and 16 (the first NaN
                    in the upper half-wave, a later NaN in the lower one: the exchange decides between two NaNs by the row), head 1
                    row 44 (upper half-wave of the second M-tile, the lower half-wave holds numbers only: NaN against a number in the
                    exchange, after a finite maximum from tile 0), head 2 row 104 (second LDS stage), head 3 rows 130 and 133 (third).
  tiny              bf16 / fp32 keys x 2^-66: every x^2 is an fp32 subnormal (queries x 2^20 keep the ThinK product in range); fp16
                    keys x 2^-18: fp16 subnormals.  The norms and channel scores are non-zero in at least half of the rows /
                    channels, so a device that flushes denormals differs visibly.  The `zeros` variant also zeroes every second key
                    channel: exactly-zero scores in at least n_prune + 8 channels (the tie order among zeros).

The cosines are no output of the oracle: the conditions that need them read torch_cosines, the restatement's matrix, whose first
maximum is compared with the oracle's pivots by test_stage_regimes_cpu.py.

References: torch_merge / torch_think / torch_l2norm — restatements, written for this repository, of the reference's merge_kv,
key_pruner_query_driven and L2NormCluster arithmetic in live torch CPU operations, optionally wrong on purpose (FAULTS) for the
mutant tests — and oracle.cam_merge.
"""
import functools
from collections import namedtuple

import torch

from kvcache_factory_amd import synth

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
_DT_NAME = {BF16: "bf16", FP16: "fp16", FP32: "fp32"}
F32_MIN_NORMAL = 2.0 ** -126

MERGE, THINK, L2NORM, CAM = "merge", "think", "l2norm", "cam"
THINK_ROWS, THINK_RECENT = 200, 32        # ThinK runs on the first 200 key rows of every query head, the last 32 kept whole
CAM_START = 16                            # CAM's start budget
MIN_TIES = 32                             # duplicates: dropped tokens per head and kind of tie


class Spec(namedtuple("Spec", "regime variant stages dtype D Hq Hkv L W n_keep rows ratio seed")):
    """stages: which of merge / think / l2norm / cam the spec feeds; rows: the L2Norm budget; ratio: ThinK's pruned share."""
    __slots__ = ()

    @property
    def name(self):
        v = f"-{self.variant}" if self.variant else ""
        return f"{self.regime}{v}-{_DT_NAME[self.dtype]}-D{self.D}-H{self.Hq}x{self.Hkv}-L{self.L}-W{self.W}-k{self.n_keep}"

    @property
    def n_prune(self):
        return int(self.D * self.ratio)


def _s(regime, variant, stages, dtype, D, Hq, Hkv, L, W, n_keep, rows, ratio, seed):
    return Spec(regime, variant, tuple(stages.split()), dtype, D, Hq, Hkv, L, W, n_keep, rows, ratio, seed)


# Shapes: the smallest that meet the conditions.  clustered: the count of the cluster's kept row is L - Hq * n_keep - W + 1 = 281 /
# 515 / 2585, odd and beyond 256 (bf16) / 2048 (fp16).  duplicates: n_keep + W = 144 = two full LDS stages and a partial one.
# zero_rows: L = 700 puts zero rows 693 in the window and among both the selected and the dropped prefix rows.
GRID = [
    _s("clustered", "", "merge", BF16, 128, 4, 2, 300, 8, 3, 0, 0.4, 101),
    _s("clustered", "", "merge", BF16, 128, 2, 2, 524, 8, 1, 0, 0.4, 102),
    _s("clustered", "", "merge", FP16, 128, 4, 2, 2600, 8, 2, 0, 0.4, 103),
    _s("outlier_channels", "", "merge think l2norm cam", BF16, 128, 4, 2, 300, 8, 40, 40, 0.4, 111),
    _s("outlier_channels", "", "merge think l2norm cam", FP16, 128, 4, 2, 300, 8, 40, 40, 0.4, 112),
    _s("outlier_channels", "", "think l2norm cam", FP32, 64, 4, 2, 300, 8, 40, 40, 0.3, 113),
    _s("outlier_channels", "", "think l2norm cam", BF16, 64, 2, 2, 300, 32, 40, 300, 0.5, 114),
    _s("duplicates", "", "merge l2norm", BF16, 128, 4, 2, 520, 8, 136, 20, 0.4, 121),
    _s("duplicates", "", "merge l2norm", FP16, 128, 2, 2, 520, 8, 136, 20, 0.4, 122),
    _s("overflow", "cut_in_infs", "merge think l2norm cam", FP16, 128, 4, 2, 300, 8, 8, 260, 0.4, 131),
    _s("overflow", "cut_in_nans", "think l2norm cam", FP16, 64, 4, 2, 300, 8, 8, 260, 0.8, 132),
    _s("zero_rows", "", "merge l2norm", BF16, 128, 4, 2, 700, 8, 40, 40, 0.4, 141),
    _s("zero_rows", "", "merge l2norm", FP16, 128, 4, 2, 700, 8, 40, 40, 0.4, 142),
    _s("zero_rows", "planted", "merge", BF16, 128, 4, 2, 700, 8, 136, 40, 0.4, 143),
    _s("zero_rows", "planted", "merge", FP16, 128, 4, 2, 700, 8, 136, 40, 0.4, 144),
    _s("tiny", "", "merge think l2norm", BF16, 128, 4, 2, 300, 8, 40, 40, 0.4, 151),
    _s("tiny", "", "merge l2norm", FP16, 128, 4, 2, 300, 8, 40, 40, 0.4, 152),
    _s("tiny", "", "think l2norm", FP32, 64, 4, 2, 300, 8, 40, 40, 0.3, 153),
    _s("tiny", "", "think l2norm", BF16, 64, 2, 2, 300, 8, 40, 40, 0.5, 154),
    _s("tiny", "zeros", "think", BF16, 128, 4, 2, 300, 8, 40, 40, 0.4, 155),
]


def specs(stage=None, regime=None):
    return [s for s in GRID if (stage is None or stage in s.stages) and (regime is None or s.regime == regime)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
DUP_KEPT = {0: (2, 66, 122), 1: (8, 40), 2: (72, 76)}      # prototype -> slots j of idx (kept key row r = W + j, W = 8):
#   prototype 0 at r = 10, 74, 130 (three LDS stages), 1 at r = 16, 48 (two M-tiles of stage 0), 2 at r = 80, 84 (half-waves)
DUP_DROPPED = {0: range(30, 64), 1: range(64, 98), 2: range(98, 132)}            # 34 dropped copies of each prototype
DUP_KEPT_POS = {0: (20, 21, 22), 1: (23, 24), 2: (25, 26)}                       # where the kept copies sit in the sequence
DUP_POOL = 140                                                                   # the other slots are drawn from [140, L - W)


ZERO_PLANTED = {0: (12, 16), 1: (44,), 2: (104,), 3: (130, 133)}      # zero_rows-planted: head -> kept key rows r that are zero


def _random_idx(spec, lo=0):
    """[Hq, n_keep] distinct positions per head in [lo, L - W), seeded."""
    n = spec.L - spec.W - lo
    order = synth.normal((spec.Hq, n), spec.seed, 5).argsort(dim=-1)
    return (order[:, :spec.n_keep] + lo).contiguous()


def key_transform(regime, k, dtype, variant=""):
    """The regimes that only reshape synth's keys k [1, Hkv, L, D] (fp32) -> dtype: outlier_channels, zero_rows, overflow, tiny."""
    k = k.clone()
    if regime == "outlier_channels":
        k[..., 5] += 40.0
        k[..., 77 % k.shape[-1]] -= 25.0
    elif regime == "zero_rows":
        k[:, :, ::7] = 0.0
        if variant == "planted":                                                 # ... but for the window (W = 8)
            k[:, :, -8:] = torch.where(k[:, :, -8:].abs().sum(-1, keepdim=True) == 0, torch.ones_like(k[:, :, -8:]), k[:, :, -8:])
    elif regime == "overflow":
        k *= 3000.0
        k[:, :, ::5] *= 4.0
        k[..., ::3] = 0.0
    elif regime == "tiny":
        k *= 2.0 ** -18 if dtype == FP16 else 2.0 ** -66
        if variant == "zeros":
            k[..., ::2] = 0.0
    return k.to(dtype)


def clustered_keys(Hq, Hkv, L, D, W, n_keep, dtype, seed):
    """(k [1, Hkv, L, D] dtype, idx [Hq, n_keep]): keys c + 0.3 n; head h keeps cluster row 100 + 17 h in slot h % n_keep and
    planted rows (-c + 0.3 n, like the window rows) in its other slots."""
    c = synth.normal((1, Hkv, 1, D), seed, 3)
    k = c + 0.3 * synth.normal((1, Hkv, L, D), seed, 1)
    idx = torch.empty(Hq, n_keep, dtype=torch.int64)
    away = list(range(L - W, L))
    for h in range(Hq):
        planted = [10 + 5 * h + i for i in range(n_keep - 1)]
        away += planted
        planted.insert(h % n_keep, 100 + 17 * h)
        idx[h] = torch.tensor(planted)
    k[:, :, away] -= 2.0 * c
    return k.to(dtype), idx


@functools.lru_cache(maxsize=None)
def inputs(spec):
    """dict(q [1, Hq, L, D] in the model's memory order, k, v [1, Hkv, L, D], idx int64 [Hq, n_keep], mask uint8
    [Hq, L - W - CAM_START]) of a spec, on the CPU.  Cached: treat as read-only."""
    Hq, Hkv, L, D, W, dt = spec.Hq, spec.Hkv, spec.L, spec.D, spec.W, spec.dtype
    q = synth.normal((1, L, Hq, D), spec.seed, 0)
    k = synth.normal((1, Hkv, L, D), spec.seed, 1)
    v = synth.normal((1, Hkv, L, D), spec.seed, 2)
    idx = _random_idx(spec)
    mask = (synth.normal((Hq, L - W - CAM_START), spec.seed, 4) > 0).to(torch.uint8)
    if spec.regime == "clustered":
        k, idx = clustered_keys(Hq, Hkv, L, D, W, spec.n_keep, dt, spec.seed)
        v = v * 8.0
    elif spec.regime == "duplicates":
        proto = 0.25 * synth.normal((Hkv, 3, D), spec.seed, 3)
        idx = _random_idx(spec, DUP_POOL)
        for p in range(3):
            k[0, :, list(DUP_DROPPED[p]) + list(DUP_KEPT_POS[p])] = proto[:, p, None]
            for j, pos in zip(DUP_KEPT[p], DUP_KEPT_POS[p]):
                idx[:, j] = pos
        k = k.to(dt)
    else:
        k = key_transform(spec.regime, k, dt, spec.variant)
    if spec.regime == "zero_rows" and spec.variant == "planted":
        pool = torch.tensor([p for p in range(L - W) if p % 7])                 # every selected row non-zero ...
        idx = pool[synth.normal((Hq, len(pool)), spec.seed, 5).argsort(dim=-1)[:, :spec.n_keep]]
        nxt = 7
        for h, rows in ZERO_PLANTED.items():                                     # ... except the planted slots
            for r in rows:
                idx[h, r - W] = nxt
                nxt += 7
    if spec.regime == "outlier_channels":
        v = v * 30.0
    if spec.regime == "overflow":
        q, v = q * 300.0, v * 10000.0
        mask = torch.ones_like(mask)
    if spec.regime == "tiny" and THINK in spec.stages:
        q = q * 2.0 ** 20
    return dict(q=q.to(dt).transpose(1, 2), k=k, v=v.to(dt), idx=idx.contiguous(), mask=mask.contiguous())


def expand(spec, t):
    return t.repeat_interleave(spec.Hq // spec.Hkv, 1) if spec.Hq != spec.Hkv else t


def think_keys(spec, k):
    """The compressed keys ThinK sees here: the first THINK_ROWS rows of every query head, dense."""
    return expand(spec, k)[:, :, :THINK_ROWS].contiguous()


# ---- the oracle on a spec (cached: one reference per spec, shared by the tests, left unchanged) -----------------------------------
@functools.lru_cache(maxsize=None)
def oracle_merge(spec):
    from oracle import kvc_oracle as O
    x = inputs(spec)
    return O.merge_pivot(x["k"], x["v"], x["idx"], spec.W)                        # K', V', pivots


@functools.lru_cache(maxsize=None)
def oracle_think(spec):
    from oracle import kvc_oracle as O
    x = inputs(spec)
    return O.think_prune(think_keys(spec, x["k"]), x["q"], THINK_RECENT, spec.ratio)   # pruned, recent, keep, scores


@functools.lru_cache(maxsize=None)
def oracle_l2norm(spec):
    from oracle import kvc_oracle as O
    x = inputs(spec)
    return O.l2norm(x["k"], x["v"], spec.rows, spec.Hq)                           # K', V', idx, norms


@functools.lru_cache(maxsize=None)
def oracle_cam(spec):
    from oracle import kvc_oracle as O
    x = inputs(spec)
    return O.cam_merge(expand(spec, x["v"]), x["mask"], spec.W, CAM_START)


# ---- references: the reference's arithmetic in live torch CPU operations, optionally wrong on purpose ----------------------------
FAULTS = ("count_unrounded", "count_sticky", "last_max", "nan_smallest", "nan_old_exchange", "flush_squares")
TARGET = {"count_unrounded": "clustered", "count_sticky": "clustered", "last_max": "duplicates", "nan_smallest": "zero_rows", "nan_old_exchange": "zero_rows",
          "flush_squares": "tiny"}


def _norm(x, fault=None):
    """torch.norm over the last dimension, kept; flush_squares: every x^2 below the smallest normal fp32 counts as 0."""
    if fault != "flush_squares":
        return torch.norm(x, dim=-1, keepdim=True)
    sq = x.float() * x.float()
    sq = torch.where(sq < F32_MIN_NORMAL, torch.zeros_like(sq), sq)
    return sq.sum(-1, keepdim=True).sqrt().to(x.dtype)


def _merge_operands(spec, k, v, idx):
    """(dropped K, dropped V, kept K [window, selected], kept V [selected, window]) as the reference lays them out: a position is
    dropped when NO head selected it, the window included."""
    kx, vx = expand(spec, k), expand(spec, v)
    L, D = kx.shape[2], kx.shape[3]
    taken = torch.zeros(L, dtype=torch.bool)
    taken[idx.flatten()] = True
    drop = (~taken).nonzero().flatten()
    ix = idx[None, :, :, None].expand(1, spec.Hq, idx.shape[1], D)
    kept_k = torch.cat([kx[:, :, -spec.W:], kx.gather(2, ix)], dim=2)
    kept_v = torch.cat([vx.gather(2, ix), vx[:, :, -spec.W:]], dim=2)
    return kx[:, :, drop], vx[:, :, drop], kept_k, kept_v


def torch_cosines(spec, fault=None):
    """The dtype cosine matrix [Hq, drop_len, n_keep + W] of a spec: unit rows (x / norm) of the dropped keys times those of the
    kept keys, transposed."""
    x = inputs(spec)
    dk, _, kk, _ = _merge_operands(spec, x["k"], x["v"], x["idx"])
    return ((dk / _norm(dk, fault)) @ (kk / _norm(kk, fault)).transpose(-1, -2))[0]


def first_max(cos, fault=None):
    """torch.max's column per row: the first maximum, NaN above every number.  last_max / nan_smallest / nan_old_exchange: wrong on
    purpose."""
    if fault == "last_max":
        return cos.shape[-1] - 1 - cos.flip(-1).max(dim=-1).indices
    if fault == "nan_smallest":
        return torch.nan_to_num(cos.float(), nan=float("-inf")).max(dim=-1).indices
    if fault == "nan_old_exchange":
        # merge_pivot_kernel's two half-waves: rows r % 8 < 4 and r % 8 >= 4 of every 8-row block.  Each orders NaN as torch.max
        # does; the pair is then joined by a rule that knows no NaN: the upper half's (value, row) replaces the lower half's
        # only if value > or (value == and row <), so an upper NaN never wins and a lower NaN is never replaced.
        c = cos.float()
        rows = torch.arange(c.shape[-1])
        lo, hi = rows[rows % 8 < 4], rows[rows % 8 >= 4]
        i0, i1 = c[..., lo].max(dim=-1).indices, c[..., hi].max(dim=-1).indices
        r0, r1 = lo[i0], hi[i1]
        v0, v1 = c.gather(-1, r0[..., None])[..., 0], c.gather(-1, r1[..., None])[..., 0]
        return torch.where((v1 > v0) | ((v1 == v0) & (r1 < r0)), r1, r0)
    return cos.max(dim=-1).indices


def torch_merge(spec, fault=None):
    """merge_kv(..., "pivot") restated: (K' [1, Hq, R, D], V', pivots int64 [Hq, drop_len]).  Without a fault the mean is torch's
    own scatter_reduce('mean', include_self=True); the count faults take its 'sum' and divide by their own count (count_unrounded:
    the exact count; count_sticky: a count advanced by dtype additions, which stops at 256 in bf16 and 2048 in fp16) — with the
    right count that path gives scatter_reduce's mean bit for bit (test_stage_regimes_cpu.py checks it)."""
    x = inputs(spec)
    dk, dv, kk, vk = _merge_operands(spec, x["k"], x["v"], x["idx"])
    cos = (dk / _norm(dk, fault)) @ (kk / _norm(kk, fault)).transpose(-1, -2)
    piv = first_max(cos, fault)
    px = piv[..., None].expand(-1, -1, -1, dk.shape[-1])
    outs = []
    for dropped, kept in ((dk, kk), (dv, vk)):
        merged = (dropped + kept.gather(2, px)) / 2
        if fault not in ("count_unrounded", "count_sticky", "count_rounded"):
            outs.append(torch.scatter_reduce(kept, 2, px, merged, reduce="mean", include_self=True))
            continue
        total = torch.scatter_reduce(kept, 2, px, merged, reduce="sum", include_self=True)
        cnt = torch.ones(piv.shape[:2] + (kept.shape[2],)).scatter_add_(2, piv, torch.ones(piv.shape))
        if fault == "count_rounded":
            cnt = cnt.to(kept.dtype).float()
        elif fault == "count_sticky":
            cnt = cnt.clamp(max=256.0 if kept.dtype == BF16 else 2048.0)
        outs.append((total.float() / cnt[..., None]).to(kept.dtype))
    return outs[0], outs[1], piv[0]


def torch_think(spec, fault=None):
    """key_pruner_query_driven restated: channel score = mean over the last 32 query rows of q^2 times the mean over the rows of
    k^2, the n_prune smallest channels dropped from all but the recent rows.  Returns (pruned, recent, keep bool [1, H, D], scores)."""
    x = inputs(spec)
    kc, q = think_keys(spec, x["k"]), x["q"]
    S, D = kc.shape[2], kc.shape[3]

    def sq(t):
        p = torch.pow(t, 2)
        if fault == "flush_squares":
            p = torch.where(p.float() < F32_MIN_NORMAL, torch.zeros_like(p), p)
        return p
    score = sq(q[:, :, -32:]).mean(dim=2) * sq(kc).mean(dim=2)
    low = torch.topk(score, spec.n_prune, dim=-1, largest=False).indices
    gone = torch.zeros(score.shape, dtype=torch.bool).scatter_(-1, low, True)
    head = kc[:, :, :S - THINK_RECENT]
    pruned = head[~gone[:, :, None].expand(-1, -1, S - THINK_RECENT, -1)].reshape(1, -1, S - THINK_RECENT, D - spec.n_prune)
    return pruned, kc[:, :, S - THINK_RECENT:], ~gone, score[0]


def torch_l2norm(spec, fault=None):
    """L2NormCluster's kept branch restated: (indices [Hq, rows] = the head of the ascending argsort of the key norms, norms)."""
    k = expand(spec, inputs(spec)["k"])
    norms = _norm(k, fault)[0, :, :, 0] if fault else torch.norm(k, p=2, dim=-1)[0]
    return norms.argsort(dim=-1)[:, :spec.rows], norms


# ---- conditions -----------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(a, b):
    """Bit for bit, NaNs equal as NaNs whatever their payload."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return bool(torch.equal(a, b))
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(bits(a)[~na], bits(b)[~nb]))


def differing(a, b):
    """Number of elements that differ in the sense of `same`."""
    if not a.dtype.is_floating_point:
        return int((a != b).sum())
    na, nb = torch.isnan(a), torch.isnan(b)
    return int(((na != nb) | (~na & ~nb & (bits(a) != bits(b)))).sum())


def _tie_kinds(r_sets):
    """r_sets: bool [M, R] — the kept rows at which a dropped token attains its maximum.  Per kind of tie, the number of tokens
    with two such rows (stages: different 64-row stages; tiles: one stage, different 32-row tiles; halves: rows r and r + 4 of
    one 8-row block, r % 8 < 4)."""
    M, R = r_sets.shape
    rows = torch.arange(R)
    n_stage = (R + 63) // 64
    st = torch.stack([r_sets[:, rows // 64 == s].any(-1) for s in range(n_stage)], -1)
    stages = int((st.sum(-1) >= 2).sum())
    tiles = torch.zeros(M, dtype=torch.bool)
    for s in range(n_stage):
        a, b = r_sets[:, (rows // 64 == s) & (rows % 64 < 32)].any(-1), r_sets[:, (rows // 64 == s) & (rows % 64 >= 32)].any(-1)
        tiles |= a & b
    lo = rows[(rows % 8 < 4) & (rows + 4 < R)]
    halves = int((r_sets[:, lo] & r_sets[:, lo + 4]).any(-1).sum())
    return dict(stages=stages, tiles=int(tiles.sum()), halves=halves)


def conditions(spec):
    """Check the regime's conditions on the reference outputs of a spec; return the counts (minima over the heads)."""
    x = inputs(spec)
    out = {}
    kf = x["k"].float()
    if MERGE in spec.stages:
        ko, vo, piv = oracle_merge(spec)
        R = spec.n_keep + spec.W
        counts = torch.stack([torch.bincount(p.long(), minlength=R) for p in piv]) + 1          # [Hq, R], include_self
        out.update(drop_len=piv.shape[1], count_max=int(counts.max()))
    if spec.regime == "clustered":
        unrep = counts.float().to(spec.dtype).float() != counts.float()
        chunks = piv[:, :piv.shape[1] // 64 * 64].view(spec.Hq, -1, 64)
        full = (chunks == chunks[:, :, :1]).all(-1).sum(-1)
        out.update(count_min_over_heads=int(counts.max(-1).values.min()), unrepresentable_rows_min=int(unrep.sum(-1).min()),
                   full_chunks_min=int(full.min()), full_chunks_of=chunks.shape[1])
        assert int(unrep.sum(-1).min()) >= 1, out
        assert int(counts[unrep].min()) >= (257 if spec.dtype == BF16 else 2049), out
        assert int(full.min()) >= 1, out
    if spec.regime == "duplicates":
        cos = torch_cosines(spec).float()
        kinds = [_tie_kinds(c == c.max(-1, keepdim=True).values) for c in cos]
        for kind in ("stages", "tiles", "halves"):
            out[f"ties_{kind}_min"] = min(kd[kind] for kd in kinds)
            assert out[f"ties_{kind}_min"] >= MIN_TIES, out
        assert spec.n_keep + spec.W > 128
        _, _, idx, norms = oracle_l2norm(spec)
        srt = norms.float().sort(dim=-1).values
        out.update(norm_ties_across_cut=int((srt[:, spec.rows - 1] == srt[:, spec.rows]).sum()))
        assert out["norm_ties_across_cut"] == spec.Hq, out
    if spec.regime == "overflow":
        assert spec.dtype == FP16
        _, _, _, norms = oracle_l2norm(spec)
        out.update(inf_norms=int(torch.isinf(norms).sum()))
        assert out["inf_norms"] > 0, out
        _, _, keep, sc = oracle_think(spec)
        gone = ~keep[0]
        for nm, m in (("inf", torch.isinf(sc)), ("nan", torch.isnan(sc))):
            out[f"{nm}_pruned_min"], out[f"{nm}_kept_min"] = int((m & gone).sum(-1).min()), int((m & ~gone).sum(-1).min())
        assert int((torch.isinf(sc) | torch.isnan(sc)).sum()) == sc.numel(), out
        assert min(out["inf_pruned_min"], out["nan_kept_min"]) > 0, out                      # infs are pruned first, NaNs last
        if spec.variant == "cut_in_infs":                                                    # infs on both sides of the boundary
            assert out["inf_kept_min"] > 0 and out["nan_pruned_min"] == 0, out
        else:                                                                                # cut_in_nans: NaNs on both sides
            assert spec.variant == "cut_in_nans" and out["nan_pruned_min"] > 0 and out["inf_kept_min"] == 0, out
        if MERGE in spec.stages:
            out.update(inf_in_merged_k=int(torch.isinf(ko).sum()))
            assert out["inf_in_merged_k"] > 0, out
        out.update(nonfinite_in_cam=int((~torch.isfinite(oracle_cam(spec))).sum()))
        assert out["nonfinite_in_cam"] > 0, out                                            # the recurrence itself overflows
    if spec.regime == "zero_rows":
        nan = torch.isnan(torch_cosines(spec))                                               # [Hq, M, R]
        all_nan = nan.all(-1).sum(-1)
        part = (nan.any(-1) & ~nan.all(-1)).sum(-1)
        out.update(all_nan_tokens_min=int(all_nan.min()), partly_nan_tokens_min=int(part.min()), nan_columns_min=int(nan.all(1).sum(-1).min()))
        assert int(all_nan.min()) >= 1 and int(part.min()) >= 1, out
        sel_zero = (kf[0, :, :, :].abs().sum(-1) == 0)                                       # zero rows among kept and dropped
        taken = torch.zeros(spec.L, dtype=torch.bool)
        taken[x["idx"].flatten()] = True
        assert bool((sel_zero[:, taken]).any()) and bool((sel_zero[:, ~taken]).any())
        cols = nan.all(1)                                                                    # [Hq, R]: the whole NaN columns
        first = [int(c.nonzero()[0]) for c in cols]
        out.update(first_nan_column_per_head=first, pivot_values=sorted({int(p) for p in oracle_merge(spec)[2].unique()})[:8])
        if spec.variant == "planted":
            assert not bool(cols[:, :spec.W].any()), out                                     # no zero row in the window
            later_lower = [bool((cols[h, f + 1:] & (torch.arange(f + 1, cols.shape[1]) % 8 < 4)).any()) for h, f in enumerate(first)]
            lower_any = [bool((cols[h] & (torch.arange(cols.shape[1]) % 8 < 4)).any()) for h in range(spec.Hq)]
            kinds = dict(upper_half_then_lower_nan=sum(f % 8 >= 4 and later_lower[h] for h, f in enumerate(first)),
                         upper_half_lower_finite=sum(f % 8 >= 4 and not lower_any[h] for h, f in enumerate(first)),
                         second_tile=sum(f % 64 >= 32 for f in first), later_stage=sum(f >= 64 for f in first))
            out.update(heads_with=kinds)
            assert all(n >= 1 for n in kinds.values()), out
            assert all(int(part[h]) >= 1 for h in range(spec.Hq)), out                       # tokens that reach that column, per head
    if spec.regime == "tiny":
        if spec.dtype == FP16:
            assert float(kf.abs().max()) < 2.0 ** -14, "fp16 keys must be fp16 subnormals"
        else:
            assert float((kf * kf).max()) < F32_MIN_NORMAL, "every x^2 must be an fp32 subnormal"
        if L2NORM in spec.stages:
            _, _, _, norms = oracle_l2norm(spec)
            out.update(nonzero_norms=int((norms.float() != 0).sum()), of_norms=norms.numel())
            assert out["nonzero_norms"] * 2 >= norms.numel(), out
        if THINK in spec.stages:
            _, _, keep, sc = oracle_think(spec)
            zeros = (sc.float() == 0).sum(-1)
            out.update(nonzero_scores=int((sc.float() != 0).sum()), of_scores=sc.numel(), zero_scores_min=int(zeros.min()))
            if spec.variant == "zeros":
                assert int(zeros.min()) >= spec.n_prune + 8, out
            else:
                assert out["nonzero_scores"] * 2 >= sc.numel(), out
    return out
