"""The stages that follow scoring — pivot merge, ThinK, L2Norm, the CAM value recurrence — on the regimes of stage_ref.py, on the
CPU: every spec meets its regime's conditions, the oracle equals live torch operations bit for bit on every spec (NaNs equal as
NaNs), and the comparison rejects restatements that are wrong on purpose.  test_stage_regimes_gpu.py runs the same GRID through the
kernels against the same oracle.
"""
import pytest
import torch

import stage_ref as S


def _of(stage=None, regime=None):
    sel = S.specs(stage, regime)
    return pytest.mark.parametrize("spec", sel, ids=[s.name for s in sel])


@_of()
def test_spec_meets_its_conditions(oracle, spec):
    """A spec that misses a condition of its regime is an input error: it fails here, and gets another seed or size."""
    print(spec.name, S.conditions(spec))


def test_grid_covers_the_issue():
    """One GRID for both files: GQA 4 x 2 and a non-GQA spec, both 16-bit dtypes through the merge, all three through ThinK and
    L2Norm, both head dims outside the merge, L within [300, 2600]."""
    assert {(s.Hq, s.Hkv) for s in S.GRID} >= {(4, 2), (2, 2)}
    assert all(300 <= s.L <= 2600 for s in S.GRID)
    assert all(s.D == 128 and s.dtype != S.FP32 for s in S.specs(S.MERGE))
    for stage in (S.THINK, S.L2NORM):
        assert {s.dtype for s in S.specs(stage)} == {S.BF16, S.FP16, S.FP32} and {s.D for s in S.specs(stage)} == {64, 128}
    assert {s.regime for s in S.specs(S.MERGE)} == {"clustered", "outlier_channels", "duplicates", "overflow", "zero_rows", "tiny"}
    assert {s.regime for s in S.specs(S.CAM)} == {"outlier_channels", "overflow"}
    assert all(s.dtype == S.FP16 for s in S.specs(regime="overflow"))


@_of(S.MERGE)
def test_merge_oracle_equals_live_torch(oracle, spec):
    """Pivots, K' and V' of the oracle against the torch restatement of merge_kv — with hundreds of merges into one row, tied
    cosines, inf in the output and NaN cosines.  On zero_rows this fails with an oracle that takes NaN only in column 0 (1876 of
    2212 pivots and 22 350 of 24 576 elements of K' differed in bf16 before kvco_merge_pivot ordered NaN like torch.max)."""
    ko, vo, piv = S.oracle_merge(spec)
    kt, vt, pt = S.torch_merge(spec)
    print(spec.name, "pivots differing", S.differing(piv.long(), pt), "K'", S.differing(ko, kt), "V'", S.differing(vo, vt))
    assert S.same(piv.long(), pt)
    assert S.same(ko, kt) and S.same(vo, vt)


@_of(S.MERGE)
def test_merge_count_harness_equals_scatter_mean(spec):
    """The path the count mutants take (scatter 'sum', then a division by a count of their own) gives torch's 'mean' bit for bit when
    the count is the right one: what the mutants change is the count alone."""
    kt, vt, _ = S.torch_merge(spec)
    kh, vh, _ = S.torch_merge(spec, "count_rounded")
    assert S.same(kt, kh) and S.same(vt, vh)


@_of(S.THINK)
def test_think_oracle_equals_live_torch(oracle, spec):
    """Channel scores (inf, NaN, exact zeros and products of subnormal means included), keep mask, pruned and recent keys."""
    pruned, recent, keep, sc = S.oracle_think(spec)
    pt, rt, kt, st = S.torch_think(spec)
    assert S.same(sc, st)
    assert S.same(keep, kt)
    assert S.same(pruned, pt) and S.same(recent.contiguous(), rt.contiguous())


@_of(S.L2NORM)
def test_l2norm_oracle_equals_live_torch(oracle, spec):
    """Kept indices in torch's ascending order — equal norms across the cut, zero, infinite and subnormal-built norms — and, for
    the 16-bit dtypes, the norms.  fp32 norms: torch fuses its multiply-add, the last bit differs in some rows (outlier_channels
    fp32: 108 of 1200) while the indices agree; the count is printed."""
    _, _, idx, norms = S.oracle_l2norm(spec)
    it, nt = S.torch_l2norm(spec)
    print(spec.name, "norms differing", S.differing(norms, nt), "of", norms.numel())
    assert S.same(idx, it)
    if spec.dtype != S.FP32:
        assert S.same(norms, nt)


def _differs(spec, fault):
    """Does the comparison above see the fault on this spec?"""
    seen = False
    if S.MERGE in spec.stages:
        ko, vo, piv = S.oracle_merge(spec)
        kt, vt, pt = S.torch_merge(spec, fault)
        seen |= not (S.same(piv.long(), pt) and S.same(ko, kt) and S.same(vo, vt))
    if fault == "flush_squares":
        if S.THINK in spec.stages:
            seen |= not S.same(S.oracle_think(spec)[3], S.torch_think(spec, fault)[3])
        if S.L2NORM in spec.stages and spec.dtype != S.FP32:
            seen |= not S.same(S.oracle_l2norm(spec)[3], S.torch_l2norm(spec, fault)[1])
        if S.L2NORM in spec.stages:
            seen |= not S.same(S.oracle_l2norm(spec)[2], S.torch_l2norm(spec, fault)[0])
    return seen


@pytest.mark.parametrize("fault", S.FAULTS)
def test_checker_rejects_mutant(oracle, fault):
    """Each fault, applied to the restatement, is seen on at least one spec of the regime that targets it: the count kept exact
    instead of rounded to the dtype, the count advanced by dtype additions (it sticks at 256 / 2048), the last maximum instead of
    the first, NaN ordered as the smallest cosine, NaN ordered rightly within a half-wave of merge_pivot_kernel but by the old rule
    between the two (seen by the planted zero_rows specs only: in the others window column 1 is NaN and every pivot is 0 or 1),
    squares below the smallest normal fp32 flushed to zero."""
    killers = [s.name for s in S.specs(regime=S.TARGET[fault]) if _differs(s, fault)]
    print(fault, "killed by", killers)
    assert killers
    if fault == "nan_old_exchange":
        assert all("planted" in n for n in killers) and len(killers) == 2


def test_nan_rule_of_torch_max():
    """The rule the oracle and merge_pivot_kernel restate, read from live torch: the first NaN column wins, an all-NaN row gives
    column 0, and without NaN the first maximal column."""
    nan = float("nan")
    for dt in (S.BF16, S.FP16, S.FP32):
        rows = torch.tensor([[1.0, nan, 3.0, nan], [nan, nan, nan, nan], [0.5, 2.0, 2.0, 1.0], [3.0, 1.0, nan, 3.0]])
        x = torch.cat([rows, torch.zeros(4, 140)], dim=1).to(dt)                    # wider than one vector step of the reduction
        assert x.max(dim=-1).indices.tolist() == [1, 0, 1, 2]
        assert S.first_max(x).tolist() == [1, 0, 1, 2]
