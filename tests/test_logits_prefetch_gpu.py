"""The K scan's tile loop (kvc_score.hip: logits_kernel) keeps the next tile's loads in flight across the MFMA chain: the
loads are unconditional, and a ragged tile reads row L - 1 in place of the rows beyond the end.  What that re-cut could
break shows at small shapes — a one-key ragged tile, the W-key mask straddling a tile boundary, only full tiles, fewer
tiles than waves, a ragged last tile after several full ones, two and four M-tiles through the `mt` loop — so these are
small: the exact mode bit for bit against the oracle's fmaf chain, the batch entry against single calls, and in the
16-bit MFMA mode a K view whose buffer goes on with NaN rows against a contiguous copy (a column fed from a row >= L
would turn its neighbours' maxima, and with them every score, into NaN — and no byte beyond row L - 1 may be read).
"""
import pytest
import torch

import golden_util as G

pytestmark = pytest.mark.gpu

LENGTHS = [33, 40, 64, 257, 300, 1000]


def _exact_vs_oracle(kvc, oracle, dev, Hq, Hkv, L, D, W, dtype, seed, debug_mask=0):
    q, k, _ = G.synth.make_qkv(Hq, Hkv, L, D, dtype, seed)
    sc_o, lg_o, _, _ = oracle.scores(q, k, W, 7, "maxpool", want_intermediates=True,
                                     dot_mode=oracle.DOT_CHAIN, sum_mode=oracle.SUM_TORCH16)
    sc, lg, _, _ = kvc.scores(kvc.SNAPKV, q.to(dev), k.to(dev), W, 7, "maxpool", want_intermediates=True,
                              dot_mode="exact", debug_mask=debug_mask)
    assert torch.equal(G.bits(lg[0].permute(0, 2, 1).cpu()), G.bits(lg_o))
    assert torch.equal(G.bits(sc[0].cpu()), G.bits(sc_o))


@pytest.mark.parametrize("L", LENGTHS)
def test_w8_bf16_lengths_exact(kvc, oracle, gpu_device, L):
    _exact_vs_oracle(kvc, oracle, gpu_device, 4, 1, L, 128, 8, torch.bfloat16, 9100 + L)


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16), (128, torch.float32)])
def test_other_instantiations_exact(kvc, oracle, gpu_device, D, dtype):
    _exact_vs_oracle(kvc, oracle, gpu_device, 4, 1, 300, D, 8, dtype, 9200 + D)


def test_w16_two_mtiles_exact(kvc, oracle, gpu_device):
    _exact_vs_oracle(kvc, oracle, gpu_device, 4, 1, 300, 128, 16, torch.bfloat16, 9301)


def test_w32_four_mtiles_through_the_mt_loop_exact(kvc, oracle, gpu_device):
    """debug bit 9: G * W = 128 rows walked one M-tile at a time by logits_kernel, not by logits_mt4_kernel."""
    _exact_vs_oracle(kvc, oracle, gpu_device, 4, 1, 300, 128, 32, torch.bfloat16, 9302, debug_mask=512)


def test_batch_of_three_equals_single_calls(kvc, gpu_device):
    W, keep = 8, 40
    items = [[t.to(gpu_device) for t in G.synth.make_qkv(4, 1, 300, 128, torch.bfloat16, 9400 + i)] for i in range(3)]
    ks, vs, idxs = kvc.compress_batch(kvc.SNAPKV, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items],
                                      W, [keep] * 3, 7, "maxpool", return_indices=True)
    for (q, k, v), kb, vb, ib in zip(items, ks, vs, idxs):
        k1, v1, i1 = kvc.compress(kvc.SNAPKV, q, k, v, W, keep, 7, "maxpool", return_indices=True)
        assert torch.equal(ib, i1)
        assert torch.equal(G.bits(kb.cpu()), G.bits(k1.cpu())) and torch.equal(G.bits(vb.cpu()), G.bits(v1.cpu()))


@pytest.mark.parametrize("L", LENGTHS)
def test_mfma16_view_of_longer_nan_buffer(kvc, gpu_device, L):
    q, k, _ = G.synth.make_qkv(4, 1, L, 128, torch.bfloat16, 9500 + L)
    qd = q.to(gpu_device)
    big = torch.full((1, 1, L + 40, 128), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    big[:, :, :L] = k.to(gpu_device)
    view = big[:, :, :L]
    a = kvc.scores(kvc.SNAPKV, qd, view, 8, 7, "maxpool", dot_mode="mfma16")
    b = kvc.scores(kvc.SNAPKV, qd, view.clone(), 8, 7, "maxpool", dot_mode="mfma16")      # a buffer that ends at row L - 1
    assert not torch.isnan(a.float()).any()
    assert torch.equal(G.bits(a.cpu()), G.bits(b.cpu()))
