"""The stages that follow scoring, on the GPU (pytest -m gpu): kvc_merge_pivot, kvc_think_prune, kvc_l2norm_compress and
kvc_cam_merge on the regimes of stage_ref.py — counts that round in the dtype, tied cosines across LDS stages, M-tiles and
half-waves, inf and NaN norms and channel scores, NaN cosines, fp32 and fp16 subnormals — against the oracle.  No tolerances:
every comparison is bit for bit, with one allowance — a NaN equals a NaN whatever its sign and payload (0 / 0 carries the
sign bit on the host and not on the device; torch's comparisons and top-k treat all NaNs alike).
test_stage_regimes_cpu.py ties the same oracle to live torch operations on the same GRID.
"""
import time

import pytest
import torch

import stage_ref as S

pytestmark = pytest.mark.gpu

_T = {"total": 0.0}
CASE_SECONDS = 5.0                        # "a few seconds at the most" per case, as a check (measured: 0.3 s for the slowest)


@pytest.fixture(autouse=True)
def _timed():
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    _T["total"] += dt
    print(f"\n[stage regimes, GPU file so far: {_T['total']:.2f} s]")
    assert dt <= CASE_SECONDS, f"case took {dt:.2f} s"


def _of(stage):
    sel = S.specs(stage)
    return pytest.mark.parametrize("spec", sel, ids=[s.name for s in sel])


@_of(S.MERGE)
def test_merge_pivot_vs_oracle(kvc, oracle, gpu_device, spec):
    """Pivots, K' and V' GQA-native, into caller buffers whose spare rows stay zero, and on repeat_kv-expanded K / V."""
    x = S.inputs(spec)
    ko_o, vo_o, piv_o = S.oracle_merge(spec)
    idx = x["idx"][None].contiguous().to(gpu_device)
    R = spec.n_keep + spec.W
    runs = [(x["k"], x["v"], True)]
    if spec.Hq != spec.Hkv:
        runs.append((S.expand(spec, x["k"]).contiguous(), S.expand(spec, x["v"]).contiguous(), False))
    for k, v, buffers in runs:
        out = None
        if buffers:
            out = tuple(torch.zeros(1, spec.Hq, R + 3, 128, dtype=spec.dtype, device=gpu_device) for _ in range(2))
        ko, vo, piv = kvc.merge_pivot(kvc.SNAPKV, k.to(gpu_device), v.to(gpu_device), idx, spec.W, return_pivot=True, out=out)
        assert piv.shape[2] == piv_o.shape[1]
        print(spec.name, "buffers" if buffers else "expanded", "pivots differing", S.differing(piv[0].cpu(), piv_o),
              "K'", S.differing(ko.cpu().contiguous(), ko_o), "V'", S.differing(vo.cpu().contiguous(), vo_o))
        assert S.same(piv[0].cpu(), piv_o)
        assert S.same(ko.cpu().contiguous(), ko_o) and S.same(vo.cpu().contiguous(), vo_o)
        if buffers:
            assert ko.data_ptr() == out[0].data_ptr()
            for o in out:
                assert int((S.bits(o[:, :, R:]) != 0).sum()) == 0                   # spare rows untouched


@_of(S.THINK)
def test_think_prune_vs_oracle(kvc, oracle, gpu_device, spec):
    """Channel scores, keep mask, pruned and recent keys, on a key view with spare rows per head."""
    x = S.inputs(spec)
    pruned_o, recent_o, keep_o, sc_o = S.oracle_think(spec)
    kc = S.think_keys(spec, x["k"])
    buf = torch.zeros(1, spec.Hq, S.THINK_ROWS + 9, spec.D, dtype=spec.dtype)
    buf[:, :, :S.THINK_ROWS] = kc
    kd = buf.to(gpu_device)
    pruned, recent, keep, sc = kvc.think_prune(kd[:, :, :S.THINK_ROWS], x["q"].to(gpu_device), S.THINK_RECENT, spec.ratio,
                                               return_scores=True)
    print(spec.name, "scores differing", S.differing(sc[0].cpu(), sc_o), "keep", S.differing(keep.cpu(), keep_o))
    assert S.same(sc[0].cpu(), sc_o)
    assert S.same(keep.cpu(), keep_o)
    assert S.same(pruned.cpu(), pruned_o) and S.same(recent.cpu().contiguous(), recent_o.contiguous())
    assert int((S.bits(kd[:, :, S.THINK_ROWS:]) != 0).sum()) == 0


@_of(S.L2NORM)
def test_l2norm_vs_oracle(kvc, oracle, gpu_device, spec):
    """Norms, the kept indices in torch's ascending order and K' / V', GQA-native."""
    x = S.inputs(spec)
    ko_o, vo_o, idx_o, norms_o = S.oracle_l2norm(spec)
    ko, vo, idx, norms = kvc.l2norm_compress(x["k"].to(gpu_device), x["v"].to(gpu_device), spec.rows, n_q_heads=spec.Hq,
                                             return_indices=True, return_norms=True)
    print(spec.name, "norms differing", S.differing(norms[0].cpu(), norms_o), "indices", S.differing(idx[0].cpu(), idx_o))
    assert S.same(norms[0].cpu(), norms_o)
    assert S.same(idx[0].cpu(), idx_o)
    assert S.same(ko.cpu(), ko_o) and S.same(vo.cpu(), vo_o)


@_of(S.CAM)
def test_cam_merge_vs_oracle(kvc, oracle, gpu_device, spec):
    """The value recurrence given a mask (overflow: all ones), in place on one value copy per query head."""
    x = S.inputs(spec)
    want = S.oracle_cam(spec)
    vd = S.expand(spec, x["v"]).contiguous().to(gpu_device)
    kvc.cam_merge(vd, x["mask"][None].contiguous().to(gpu_device), spec.W, S.CAM_START)
    print(spec.name, "values differing", S.differing(vd.cpu(), want))
    assert S.same(vd.cpu(), want)
