"""The window-8 softmax stage with two heads per CU (softmax_pool_pair_kernel; pytest -m gpu).

The stage's default one-workgroup-per-head form at W = 8, 16-bit dtypes and 1 024 <= L <= 8 064 recomputes its exponentials in the
second pass from the raw logits it holds, so that two workgroups fit a CU; debug_stage_mask bit 14 selects the form that keeps
them in registers (softmax_pool_ws_kernel).  Same arithmetic in the same order: scores, row maxima and row sums are compared bit
for bit — new form against old form against the two-kernel split form, and against the oracle's product arithmetic.  No tolerance.

Lengths: with WK = 896 worker threads per workgroup (a stage is 896 keys), 1024 is the smallest L of the dispatch, 2 WK fills its
last stage exactly, 2 WK + 1 leaves a last stage of one key, 2 WK + 17 one with L % 16 != 0, 8000 is the benchmark's length, 8063
and 8064 are the two largest.  (The spread / negative regimes of score_ref.py run in bf16: scale 100 is outside fp16's range.)
"""
import ctypes

import pytest
import torch

import golden_util as G
import score_ref as S
from kvcache_factory_amd import synth

pytestmark = pytest.mark.gpu

KEEP = 1 << 14                                   # debug_stage_mask bit 14: the one-head-per-CU form
WK = 896                                         # worker threads per workgroup of softmax_pool_pair_kernel<DT, 1024>
LENGTHS = [1024, 2 * WK, 2 * WK + 1, 2 * WK + 17, 8000, 8063, 8064]
POOLS = [("maxpool", 7, L) for L in LENGTHS] + [(p, ks, L) for p, ks in (("avgpool", 5), (None, 7)) for L in (2 * WK + 17, 8063)]
HQ, HKV = 4, 2

_IN = {}


def _inputs(dtype, D, L, dev):
    key = (dtype, D, L)
    if key not in _IN:
        q, k, _ = synth.make_qkv(HQ, HKV, L, D, dtype, 4400 + L + D, device=dev)
        _IN[key] = (q, k)
    return _IN[key]


def _i32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b, what):
    assert torch.equal(G.bits(a[0]), G.bits(b[0])), what + ": scores"
    assert torch.equal(_i32(a[2]), _i32(b[2])), what + ": row maxima"
    assert torch.equal(_i32(a[3]), _i32(b[3])), what + ": row sums"


def _three_forms(kvc, q, k, W, kernel, pooling):
    new = kvc.scores(kvc.SNAPKV, q, k, W, kernel, pooling, want_intermediates=True, softmax_path="fused")
    old = kvc.scores(kvc.SNAPKV, q, k, W, kernel, pooling, want_intermediates=True, softmax_path="fused", debug_mask=KEEP)
    split = kvc.scores(kvc.SNAPKV, q, k, W, kernel, pooling, want_intermediates=True, softmax_path="split")
    return new, old, split


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pooling,kernel,L", POOLS, ids=["%s%d-L%d" % (p or "none", ks, L) for p, ks, L in POOLS])
def test_pair_form_equals_kept_and_split_forms(kvc, gpu_device, pooling, kernel, L, dtype, D):
    """(a) synth.make_qkv inputs: the two-heads-per-CU form, the kept-exponentials form (bit 14) and the split form agree bit for bit."""
    q, k = _inputs(dtype, D, L, gpu_device)
    new, old, split = _three_forms(kvc, q, k, 8, kernel, pooling)
    _same(new, old, "pair vs kept")
    _same(new, split, "pair vs split")


@pytest.mark.parametrize("regime,scale", [("spread", 100), ("negative", 8)])
def test_pair_form_on_wide_logit_ranges(kvc, gpu_device, regime, scale):
    """(a) score_ref regimes at L = 2 WK + 17: exponentials in the subnormal band, and negative row maxima, in the recomputed pass."""
    spec = S.Spec("snap", regime, torch.bfloat16, 128, HQ, HKV, 2 * WK + 17, 8, "maxpool", 7, 64, scale, 91)
    q, k, _ = S.inputs(spec)
    new, old, split = _three_forms(kvc, q.to(gpu_device), k.to(gpu_device), 8, 7, "maxpool")
    m = new[2].float()
    arg = new[1].float() - m[..., None, :]                      # logits [b, H, L, W] minus the row maxima [b, H, W]
    if regime == "spread":
        assert int(((arg >= S.BAND_LO) & (arg <= S.BAND_HI)).sum()) >= HQ * 8      # the regime's own condition (score_ref.py)
    else:
        assert float(m.max()) < -4.0
    _same(new, old, "pair vs kept")
    _same(new, split, "pair vs split")


@pytest.mark.parametrize("L", [1024, 2 * WK + 17, 8064])
def test_pair_form_bit_exact_vs_oracle(kvc, oracle, gpu_device, L):
    """(b) against the oracle's product arithmetic (DOT_CHAIN, SUM_TORCH16): bit-identical scores, with and without bit 14."""
    q, k = _inputs(torch.bfloat16, 128, L, gpu_device)
    sc_o = oracle.scores(q.cpu(), k.cpu(), 8, 7, "maxpool", dot_mode=oracle.DOT_CHAIN, sum_mode=oracle.SUM_TORCH16)
    for mask in (0, KEEP):
        sc = kvc.scores(kvc.SNAPKV, q, k, 8, 7, "maxpool", dot_mode="exact", softmax_path="fused", debug_mask=mask)
        assert torch.equal(G.bits(sc[0]), G.bits(sc_o)), mask


@pytest.mark.parametrize("W,L", [(8, 1023), (8, 8065), (16, 2 * WK + 17)])
def test_bit14_outside_the_dispatch(kvc, gpu_device, W, L):
    """(c) below 1 024 and beyond 8 064 keys, and at W = 16, the form does not apply: bit 14 changes nothing."""
    q, k, _ = synth.make_qkv(HQ, HKV, L, 128, torch.bfloat16, 4500 + L + W, device=gpu_device)
    a = kvc.scores(kvc.SNAPKV, q, k, W, 7, "maxpool", want_intermediates=True, softmax_path="fused")
    b = kvc.scores(kvc.SNAPKV, q, k, W, 7, "maxpool", want_intermediates=True, softmax_path="fused", debug_mask=KEEP)
    split = kvc.scores(kvc.SNAPKV, q, k, W, 7, "maxpool", want_intermediates=True, softmax_path="split")
    _same(a, b, "with vs without bit 14")
    _same(a, split, "fused vs split")


def test_batch_items_choose_the_pair_form(kvc, gpu_device):
    """(d) 4 items x 32 heads = 128 heads: the library picks the one-workgroup-per-head stage itself, over the item dimension.
    kvc_compress_batch, the same call with bit 14, and kvc_compress per item return the same K', V' and indices."""
    L, W, keep, n = 1031, 8, 64, 4
    qkv = [synth.make_qkv(32, 8, L, 128, torch.bfloat16, 4600 + i, device=gpu_device) for i in range(n)]
    ko, vo, ix = kvc.compress_batch(kvc.SNAPKV, [t[0] for t in qkv], [t[1] for t in qkv], [t[2] for t in qkv], W, [keep] * n, 7,
                                    "maxpool", "torch_cpu", return_indices=True)
    bp = kvc.BatchPlan(kvc.SNAPKV, qkv, W, [keep] * n, 7, "maxpool", "torch_cpu", want_indices=True)
    pp = kvc.Params.from_buffer_copy(bp.p)
    pp.debug_stage_mask = KEEP
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    assert bp.call(params=pp, stream=stream) == 0, kvc.lib().kvc_last_error()
    torch.cuda.synchronize(gpu_device)
    for i, (q, k, v) in enumerate(qkv):
        k1, v1, i1 = kvc.compress(kvc.SNAPKV, q, k, v, W, keep, 7, "maxpool", "torch_cpu", return_indices=True)
        for got_k, got_v, got_i, what in ((ko[i], vo[i], ix[i], "batch"), (bp.k_out[i], bp.v_out[i], bp.idx[i], "batch, bit 14")):
            assert torch.equal(got_i.cpu().view(i1.shape), i1.cpu()), (i, what)
            assert torch.equal(G.bits(got_k).view(-1), G.bits(k1).view(-1)), (i, what)
            assert torch.equal(G.bits(got_v).view(-1), G.bits(v1).view(-1)), (i, what)
