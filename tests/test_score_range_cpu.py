"""The scoring stage over the logit range, on the CPU: the regimes of score_ref.py meet their conditions, the oracle's softmax
agrees with an fp64 softmax to a derived per-element bound, its exponential agrees with torch.softmax's over the whole band of
subnormal results, the oracle in product mode agrees with the reference's arithmetic in live torch operations, and three faulty
restatements of the softmax stage are rejected by the same bound.  (DESIGN.md §4 "Scoring stage over the logit range".)
"""
import math

import numpy as np
import pytest
import torch

import golden_util as G
import score_ref as S

IDS = [s.name for s in S.GRID]
_CACHE = {}


def _case(oracle, spec):
    """(q, k, pooled scores, logits, probabilities) of a spec from the oracle in product mode; computed once, read only."""
    if spec.name not in _CACHE:
        q, k, _ = S.inputs(spec)
        sc, lg, pr, _ = S.oracle_scores(oracle, spec, q, k, want_intermediates=True)
        _CACHE[spec.name] = (q, k, sc, lg, pr)
    return _CACHE[spec.name]


def _spec(form, regime, dtype=None):
    return next(s for s in S.GRID if s.form == form and s.regime == regime and (dtype is None or s.dtype == dtype))


@pytest.mark.parametrize("spec", S.GRID, ids=IDS)
def test_regime_conditions(oracle, spec):
    """Every GRID spec meets the conditions that define its regime (counts printed: pytest -s)."""
    _, _, sc, lg, _ = _case(oracle, spec)
    print(spec.name, S.conditions(spec, lg, sc))


@pytest.mark.parametrize("spec", S.GRID, ids=IDS)
def test_probabilities_against_fp64(oracle, spec):
    """The oracle's probabilities against softmax64 of its own logits, per element:
    |p - p64| <= 1/2 ulp_dtype(p64) + 2^-17 p64 + 2^-149 (score_ref.prob_bound derives the terms).  Measured over every regime and
    dtype: the relative part stays below 0.25 x 2^-17.  With the exponential flushing to +0 from n = -126 down (before the fix)
    this fails on the spread specs of bf16 and fp32, in the band only: p64 there is up to 2^-126, the flushed result 0."""
    _, _, _, lg, pr = _case(oracle, spec)
    ok, worst = S.probs_within_bound(pr, lg, spec.dtype)
    print(spec.name, "worst |p - p64| / bound = %.3f, relative excess / 2^-17 = %.3f" % (worst, S.rel_excess(pr, lg, spec.dtype) * 2 ** 17))
    assert ok, worst


def test_exp_band_pinned_to_torch_softmax(oracle):
    """Every fp32 argument from ln 2^-150 up to -86.0 (2.36 M values): torch.softmax of the rows [0, x, x, ...] has the row sum
    exactly 1 there, so its output IS torch's exponential.  The oracle's exp_u20 must be within 32 fp32 units of it (2^-149 each in
    the subnormal range) and, both rounded to bf16, equal everywhere but on a share of at most 0.5 %, each by one bf16 unit — the
    tolerance class of test_scores_against_reference.  Measured: at most 6 units; 0.00034 % of the bf16 values differ.  (Exact
    agreement is out of reach: torch's softmax exponential is not its header's exp_u20 — above the band, too, 100 % of the fp32
    results in [-86, -80] differ from exp_u20 in the last bits — but it does underflow gradually, which is what is pinned.)"""
    lo, hi = np.float32(math.log(2.0 ** -150)), np.float32(-86.0)
    x = np.arange(hi.view(np.uint32), lo.view(np.uint32) + 1, dtype=np.uint32).view(np.float32)       # negative: bits ascend downwards
    assert x[0] == hi and x[-1] == lo and x.size > 2_300_000
    pad = (-x.size) % 15
    rows = np.concatenate([x, np.full(pad, x[-1], np.float32)]).reshape(-1, 15)
    rows = torch.from_numpy(np.concatenate([np.zeros((rows.shape[0], 1), np.float32), rows], 1))
    p = torch.softmax(rows, -1)
    assert bool((p[:, 0] == 1).all())
    want = p[:, 1:].reshape(-1)[:x.size].contiguous()
    got = oracle.exp_u20(torch.from_numpy(x.copy()))
    assert int((want == 0).sum()) == 0 and int((got == 0).sum()) == 0                   # gradual down to the last argument
    d = G.ulp_diff(got, want)
    db = G.ulp_diff(got.to(torch.bfloat16), want.to(torch.bfloat16))
    share = float((db > 0).double().mean())
    print("exp band: %d arguments, max %d fp32 units, %.2f %% differ in fp32, bf16 share %.5f %% (max %d unit)"
          % (x.size, int(d.max()), 100 * float((d > 0).double().mean()), 100 * share, int(db.max())))
    assert int(d.max()) <= 32
    assert int(db.max()) <= 1 and share <= 0.005
    # the ends: +0 from -151 ln 2 down (and for any finite argument below), 1 at 0
    ends = oracle.exp_u20(torch.tensor([-104.0, -104.7, -1000.0, -3.0e38, 0.0]))
    assert ends.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0] and not bool(torch.signbit(ends).any())


SCORED = [s for s in S.GRID if s.form in ("snap", "rows16", "h2o")]


@pytest.mark.parametrize("spec", SCORED, ids=[s.name for s in SCORED])
def test_oracle_against_live_torch(oracle, spec):
    """The oracle in product mode against the reference's arithmetic in live torch CPU operations (score_ref.torch_scores).
    bf16 / fp16: the tolerance of test_scores_against_reference (at most 1 unit, on at most max(2, 0.5 %) of the pooled scores) and
    topk indices identical in every head; fp32: every score within 32 fp32 units.  Before the fix the bf16 spread specs fail
    (scores near 1e-38 against exact zeros, and the selections that reach into them)."""
    q, k, sc, _, _ = _case(oracle, spec)
    ref = S.torch_scores(spec, q, k)
    d = G.ulp_diff(sc, ref)
    print(spec.name, "scores differing: %d of %d, max %d units" % (int((d > 0).sum()), d.numel(), int(d.max())))
    if spec.dtype == torch.float32:
        assert int(d.max()) <= 32
        return
    assert int(d.max()) <= 1 and int((d > 0).sum()) <= max(2, d.numel() // 200)
    idx, _ = oracle.topk(sc, spec.n_keep, oracle.TIES_TORCH)
    assert torch.equal(idx, ref.topk(spec.n_keep, dim=-1).indices)


MUTANTS = [("max_from_zero", next(s for s in S.GRID if s.regime == "negative" and s.scale == 32)),
           ("folded_column", _spec("snap", "edge_needle", S.BF16)), ("folded_column", _spec("snap", "edge_needle", S.FP32)),
           ("flush_below_87", _spec("snap", "spread", S.BF16)), ("flush_below_87", _spec("snap", "spread", S.FP32))]


@pytest.mark.parametrize("fault,spec", MUTANTS, ids=[f"{f}-{s.name}" for f, s in MUTANTS])
def test_faulty_softmax_restatements_are_rejected(oracle, fault, spec):
    """score_ref.softmax_np restates the softmax stage in numpy fp32.  Without a fault it passes the fp64 bound on the named spec;
    with the row maximum started from 0 (negative), a planted column folded into the maximum of rows that cannot see it
    (edge_needle) or the exponential's lower clamp at -87.0 flushing to 0 (spread) it does not — so the bound would notice each."""
    q, k, _, lg, _ = _case(oracle, spec)
    hidden = S.hidden_last_column(spec, q, k) if fault == "folded_column" else None
    good, worst_good = S.probs_within_bound(S.softmax_np(lg, spec.dtype), lg, spec.dtype)
    bad, worst_bad = S.probs_within_bound(S.softmax_np(lg, spec.dtype, fault, hidden), lg, spec.dtype)
    print(spec.name, fault, "worst / bound: clean %.3f, faulty %.3g" % (worst_good, worst_bad))
    assert good, worst_good
    assert not bad
