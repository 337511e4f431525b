"""The scoring stage over the logit range, on the GPU (pytest -m gpu): every form of the stage on the regimes of score_ref.py —
arguments of the exponential down into the band of subnormal results and below, negative row maxima, exactly-zero logits in mixed
tiles, needles on the tile and mask edges — bit for bit against the oracle's product arithmetic (dot_mode "exact" = DOT_CHAIN,
SUM_TORCH16), the forced paths against each other, and on the spread regime the selection among exactly-zero scores end to end.
test_score_range_cpu.py ties the same oracle to an fp64 softmax and to live torch operations.  (mfma16 is a tolerance mode: not here.)
"""
import pytest
import torch

import golden_util as G
import score_ref as S

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(oracle, spec):
    """Inputs of a spec and the oracle's (pooled scores, logits) for them; computed once, read only."""
    if spec.name not in _CACHE:
        q, k, v = S.inputs(spec)
        sc, lg, _, _ = S.oracle_scores(oracle, spec, q, k, want_intermediates=True)
        _CACHE[spec.name] = (q, k, v, sc, lg)
    return _CACHE[spec.name]


def _of(*forms, regime=None):
    sel = [s for s in S.GRID if s.form in forms and (regime is None or s.regime == regime)]
    return pytest.mark.parametrize("spec", sel, ids=[s.name for s in sel])


def _i32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@_of("snap", "rows16", "decode")
def test_window_forms_bit_exact_vs_oracle(kvc, oracle, gpu_device, spec):
    """Logits, row maxima, row sums and pooled scores of the window forms equal the oracle's bit for bit, on the library's own
    choice of kernels and on each forced softmax path (split / fused / fused_r2; W = 32 also the per-M-tile scan, debug bit 9)."""
    q, k, _, sc_o, lg_o = _case(oracle, spec)
    m_o, s_o = S.oracle_rowmax_rowsum(oracle, lg_o)
    qd, kd = q.to(gpu_device), k.to(gpu_device)
    runs = [dict(), dict(softmax_path="split"), dict(softmax_path="fused"), dict(softmax_path="fused_r2")]
    if spec.W == 32:
        runs.append(dict(debug_mask=512))
    for kw in runs:
        sc, lg, rmax, rsum = kvc.scores(kvc.SNAPKV, qd, kd, spec.W, spec.kernel, spec.pooling, want_intermediates=True,
                                        dot_mode="exact", **kw)
        assert torch.equal(G.bits(lg[0].permute(0, 2, 1)), G.bits(lg_o)), kw          # tolerance: 0 ulp, the mask included
        assert torch.equal(_i32(rmax[0]), _i32(m_o)), kw
        assert torch.equal(_i32(rsum[0]), _i32(s_o)), kw
        assert torch.equal(G.bits(sc[0]), G.bits(sc_o)), kw


@_of("h2o")
def test_h2o_forms_bit_exact_vs_oracle(kvc, oracle, gpu_device, spec):
    """H2O's column sums over all L rows: the fused form, the materialising kernels (debug bit 11) and their row chunks (bit 7)
    equal the oracle bit for bit — the wide form (L % 8 == 0) and the one-column form (L = 300)."""
    q, k, _, sc_o, _ = _case(oracle, spec)
    qd, kd = q.to(gpu_device), k.to(gpu_device)
    for mask in (0, 2048, 128 | 2048):
        sc = kvc.scores(kvc.H2O, qd, kd, spec.W, spec.kernel, None, dot_mode="exact", debug_mask=mask)
        assert torch.equal(G.bits(sc[0]), G.bits(sc_o)), mask


@_of("ragged")
def test_ragged_window_mean_bit_exact_vs_oracle(kvc, oracle, gpu_device, spec):
    """AdaKV's window MEAN (ragged_compress(..., return_scores=True)) equals the oracle's."""
    q, k, v, sc_o, _ = _case(oracle, spec)
    r = kvc.ragged_compress(kvc.ADAKV, q.to(gpu_device), k.to(gpu_device), v.to(gpu_device), spec.W, spec.n_keep,
                            spec.kernel, spec.pooling, return_scores=True)
    assert torch.equal(G.bits(r["scores"][0]), G.bits(sc_o))


@_of("cam")
def test_cam_plan_bit_exact_vs_oracle(kvc, oracle, gpu_device, spec):
    """CAM reads the stage's logits, row maxima and row sums back from the workspace: its window-sum scores and merge
    probabilities equal the oracle's."""
    q, k, _, _, _ = _case(oracle, spec)
    start = 32
    sc_o, prob_o = oracle.cam_plan(q, k, spec.W, start, dot_mode=oracle.DOT_CHAIN, sum_mode=oracle.SUM_TORCH16)
    sc, prob = kvc.cam_plan(q.to(gpu_device), k.to(gpu_device), spec.W, start)
    assert torch.equal(G.bits(sc[0]), G.bits(sc_o))
    assert torch.equal(G.bits(prob[0]), G.bits(prob_o))


SPREAD = [s for s in S.GRID if s.regime == "spread" and s.form in ("snap", "rows16", "h2o")]


@pytest.mark.parametrize("tie", ["torch_cpu", "canonical"])
@pytest.mark.parametrize("spec", SPREAD, ids=[s.name for s in SPREAD])
def test_spread_compress_equals_oracle(kvc, oracle, gpu_device, spec, tie):
    """spread: n_keep takes at least 8 exactly-zero pooled scores in every head and leaves at least 8 — compress in both tie modes
    returns the oracle's indices (order included) and K' / V' bytes."""
    q, k, v, _, _ = _case(oracle, spec)
    method = kvc.H2O if spec.form == "h2o" else kvc.SNAPKV
    ko, vo, idx = kvc.compress(method, q.to(gpu_device), k.to(gpu_device), v.to(gpu_device), spec.W, spec.n_keep, spec.kernel,
                               spec.pooling, tie, return_indices=True, dot_mode="exact")
    ko_o, vo_o, idx_o, _ = oracle.compress(q, k, v, spec.W, spec.n_keep, spec.kernel, spec.pooling or "avgpool",
                                           full_rows=spec.form == "h2o", dot_mode=oracle.DOT_CHAIN, sum_mode=oracle.SUM_TORCH16,
                                           tie_mode=oracle.TIES_TORCH if tie == "torch_cpu" else oracle.TIES_CANON)
    assert torch.equal(idx[0].cpu(), idx_o)
    assert torch.equal(G.bits(ko), G.bits(ko_o)) and torch.equal(G.bits(vo), G.bits(vo_o))


def test_spread_batch_dimension_and_compress_batch(kvc, oracle, gpu_device):
    """One spread spec at bsz = 2 (the spec and its head-reversed copy) and as two items of one compress_batch call: each item
    equals the oracle's result for it."""
    spec = SPREAD[0]
    q, k, v, _, _ = _case(oracle, spec)
    q2 = q.transpose(1, 2).flip(2).contiguous().transpose(1, 2)                  # heads reversed, in q's own memory order
    items = [(q, k, v), (q2, k.flip(1).contiguous(), v.flip(1).contiguous())]
    assert q2.stride() == q.stride()
    want = [oracle.compress(a, b, c, spec.W, spec.n_keep, spec.kernel, spec.pooling, dot_mode=oracle.DOT_CHAIN,
                            sum_mode=oracle.SUM_TORCH16, tie_mode=oracle.TIES_TORCH) for a, b, c in items]
    qb, kb, vb = (torch.cat([it[i] for it in items], 0).to(gpu_device) for i in range(3))
    ko, vo, idx = kvc.compress(kvc.SNAPKV, qb, kb, vb, spec.W, spec.n_keep, spec.kernel, spec.pooling, "torch_cpu",
                               return_indices=True, dot_mode="exact")
    kos, vos, idxs = kvc.compress_batch(kvc.SNAPKV, [it[0].to(gpu_device) for it in items], [it[1].to(gpu_device) for it in items],
                                        [it[2].to(gpu_device) for it in items], spec.W, [spec.n_keep] * 2, spec.kernel, spec.pooling,
                                        "torch_cpu", return_indices=True, dot_mode="exact")
    for b, (ko_o, vo_o, idx_o, _) in enumerate(want):
        assert torch.equal(idx[b].cpu(), idx_o) and torch.equal(idxs[b][0].cpu(), idx_o)
        assert torch.equal(G.bits(ko[b:b + 1]), G.bits(ko_o)) and torch.equal(G.bits(vo[b:b + 1]), G.bits(vo_o))
        assert torch.equal(G.bits(kos[b]), G.bits(ko_o)) and torch.equal(G.bits(vos[b]), G.bits(vo_o))


@_of("decode")
def test_decode_compress_split_cache_equals_compress(kvc, oracle, gpu_device, spec):
    """The split decode cache (prefix 200 rows per query head, tail 100 rows per KV head, the W queries in a ring) compressed by
    decode_compress equals compress on the materialised cache, and the oracle: scores, indices, K' / V' bytes."""
    q, k, v, _, _ = _case(oracle, spec)
    P, W, g = S.DECODE_PREFIX, spec.W, spec.Hq // spec.Hkv
    T, rs = spec.L - P, 3
    qd, kd, vd = q.to(gpu_device), k.to(gpu_device), v.to(gpu_device)
    kp, vp = kd[:, :, :P].repeat_interleave(g, 1).contiguous(), vd[:, :, :P].repeat_interleave(g, 1).contiguous()
    kt, vt = kd[:, :, P:].contiguous(), vd[:, :, P:].contiguous()
    ring = torch.roll(qd[:, :, -W:], rs, dims=2).contiguous()                     # window row w = ring row (rs + w) % W
    kb = torch.empty(1, spec.Hq, spec.n_keep + W, spec.D, dtype=spec.dtype, device=gpu_device)
    vb = torch.empty_like(kb)
    res = kvc.decode_compress(kvc.SNAPKV, ring, rs, kp, vp, P, kt, vt, T, (kb, vb), W, spec.n_keep, spec.kernel, spec.pooling,
                              "torch_cpu", return_indices=True, return_scores=True)
    ref = kvc.compress(kvc.SNAPKV, qd, kd, vd, W, spec.n_keep, spec.kernel, spec.pooling, "torch_cpu", return_indices=True,
                       return_scores=True, dot_mode="exact")
    ko_o, vo_o, idx_o, sc_o = oracle.compress(q, k, v, W, spec.n_keep, spec.kernel, spec.pooling, dot_mode=oracle.DOT_CHAIN,
                                              sum_mode=oracle.SUM_TORCH16, tie_mode=oracle.TIES_TORCH)
    for got in (res, ref):
        assert torch.equal(G.bits(got[3][0]), G.bits(sc_o)) and torch.equal(got[2][0].cpu(), idx_o)
        assert torch.equal(G.bits(got[0]), G.bits(ko_o)) and torch.equal(G.bits(got[1]), G.bits(vo_o))
