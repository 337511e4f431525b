"""select_gather_kernel (tie_mode torch_cpu, every budget in WaveHeapL's regime: 16-bit, 1 <= k <= 128, k * 64 <= n):
the exact selection and the K / V gather in one kernel.  Compared byte for byte with the separate select_exact + gather
launches that debug_stage_mask bit 13 forces: K', V', indices and, when requested, the scores."""
import ctypes

import pytest
import torch

import golden_util as G

pytestmark = pytest.mark.gpu

FORCE_SEPARATE = 8192          # debug_stage_mask bit 13


def _run(kvc, bp, mask, scores=None, stream=None):
    p = kvc.Params.from_buffer_copy(bp.p)
    p.debug_stage_mask = mask
    for t in bp.k_out + bp.v_out + (bp.idx or []):
        t.fill_(-1)
    arr = (ctypes.c_void_p * bp.n)(*[s.data_ptr() for s in scores]) if scores is not None else None
    if scores is not None:
        for s in scores:
            s.fill_(-1)
    rc = bp.call(params=p, scores_out=arr, stream=stream)
    assert rc == 0, kvc.lib().kvc_last_error().decode()
    torch.cuda.synchronize()
    out = [t.clone() for t in bp.k_out + bp.v_out + (bp.idx or [])]
    if scores is not None:
        out += [s.clone() for s in scores]
    return out


def _bits(t):
    return t if t.dtype == torch.int64 else t.view(torch.int16)       # NaN scores compare by their bits


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _compare(kvc, qkv, W, keeps, kernel=7, pooling="maxpool", outs=None, want_scores=False):
    bp = kvc.BatchPlan(kvc.SNAPKV, qkv, W, keeps, kernel, pooling, "torch_cpu", want_indices=True, outs=outs)
    scores = None
    if want_scores:
        q, k, _ = qkv[0]
        scores = [torch.empty(k.shape[0], q.shape[1], k.shape[2] - W, dtype=k.dtype, device=k.device) for _ in qkv]
    fused = _run(kvc, bp, 0, scores)
    separate = _run(kvc, bp, FORCE_SEPARATE, scores)
    _same(fused, separate)
    return bp, fused


W8_16BIT = lambda m: (m["method"] in ("snapkv", "pyramidkv") and not m["passthrough"] and m["W"] == 8          # noqa: E731
                      and m["dtype"] in ("bf16", "fp16") and m["n_keep"] * 64 <= m["L"] - m["W"] and m["n_keep"] <= 128)


@pytest.mark.parametrize("expanded", [False, True])
@pytest.mark.parametrize("name", G.names(W8_16BIT))
def test_fused_equals_separate_on_fixtures(kvc, gpu_device, name, expanded):
    m = G.MANIFEST[name]
    q, k, v = [t.to(gpu_device) for t in G.inputs(m, expanded=expanded)]
    _compare(kvc, [(q, k, v)], m["W"], [m["n_keep"]], m["kernel"], m["pooling"], want_scores=True)


@pytest.mark.parametrize("kind", ["all_equal", "plateaus", "nan"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_equals_separate_on_tie_heavy_and_nan_rows(kvc, gpu_device, kind, dtype):
    L, W, keep = 8000, 8, 120
    q, k, v = G.synth.make_qkv(32, 8, L, 128, dtype, 7, device=gpu_device)
    if kind == "all_equal":
        k = torch.zeros_like(k)
    elif kind == "plateaus":                            # few distinct keys: long runs of equal scores
        k = k[:, :, torch.arange(L, device=gpu_device) // 500 % 3].contiguous()
    else:
        k[:, :3, 1234] = float("nan")                   # NaN logits: whole rows of NaN scores in three KV heads
    _compare(kvc, [(q, k, v)], W, [keep], want_scores=True)


def test_fused_equals_separate_bsz2_odd_lengths_and_out_stride(kvc, gpu_device):
    for L, keep in ((1101, 16), (4103, 63), (8000, 120)):
        rows = [G.synth.make_qkv(32, 8, L, 128, torch.bfloat16, 90 + b, device=gpu_device) for b in range(2)]
        q, k, v = [torch.cat([r[i] for r in rows], 0).contiguous() for i in range(3)]
        _compare(kvc, [(q, k, v)], 8, [keep])
        cap = keep + 8 + 5                               # a decode cache with spare rows per head
        outs = [(torch.zeros(2, 32, cap, 128, dtype=k.dtype, device=gpu_device),
                 torch.zeros(2, 32, cap, 128, dtype=k.dtype, device=gpu_device))]
        _compare(kvc, [(q, k, v)], 8, [keep], outs=outs)


def test_fused_equals_separate_32_items_mixed_budgets(kvc, gpu_device):
    L = 8000
    keeps = [1 + (37 * i) % 120 for i in range(32)]
    qkv = [G.synth.make_qkv(32, 8, L, 128, torch.bfloat16, 200 + i, device=gpu_device) for i in range(32)]
    _compare(kvc, qkv, 8, keeps)
    _compare(kvc, qkv[:4], 32, keeps[:4])                # W = 32 takes the same kernel
    expanded = [(q, k.repeat_interleave(4, 1), v.repeat_interleave(4, 1)) for q, k, v in qkv[:4]]   # repeat_kv layout
    _compare(kvc, expanded, 8, keeps[:4])


def test_one_ineligible_item_falls_back(kvc, gpu_device):
    """k = 300 is outside WaveHeapL's regime: the whole launch takes the separate kernels, with the same results as a
    launch of the eligible items alone."""
    L = 8000
    qkv = [G.synth.make_qkv(32, 8, L, 128, torch.bfloat16, 300 + i, device=gpu_device) for i in range(3)]
    _, mixed = _compare(kvc, qkv, 8, [120, 300, 64])
    _, alone = _compare(kvc, [qkv[0], qkv[2]], 8, [120, 64])
    _same([mixed[0], mixed[2], mixed[3], mixed[5], mixed[6], mixed[8]], alone)


def test_fused_replays_from_a_hip_graph_and_repeats(kvc, gpu_device):
    L, keeps = 8000, [120, 64, 17, 120]
    qkv = [G.synth.make_qkv(32, 8, L, 128, torch.bfloat16, 40 + i, device=gpu_device) for i in range(len(keeps))]
    bp, want = _compare(kvc, qkv, 8, keeps)
    for _ in range(3):                                  # the same bits on every run
        _same(_run(kvc, bp, 0), want)
    side = torch.cuda.Stream(device=gpu_device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        bp.run(ctypes.c_void_p(side.cuda_stream))
    for _ in range(2):
        for t in bp.k_out + bp.v_out + bp.idx:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        _same([t.clone() for t in bp.k_out + bp.v_out + bp.idx], want)
