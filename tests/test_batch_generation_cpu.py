"""Batched generation over left-padded prompts of unequal length, without a GPU: the row geometry read from the attention mask,
the per-row prefill (every prompt of the batch compressed as the sequence it is alone — the kernels replaced by the oracle
stand-ins of cpu_compress.py, which take bsz = 1 items only, so anything that is not a per-row call fails outright), the cache
layer with per-row lengths in both forms, the refusals, a tiny Llama driven teacher-forced against its own solo runs, and the
argument checks of kvc_decode_step_rows."""
import ctypes

import pytest
import torch

from cpu_compress import oracle_compress, oracle_compress_batch, oracle_compress_merge, oracle_decode_step, oracle_l2norm_compress
from kvcache_factory_amd import _kvc


# ---- stand-ins -----------------------------------------------------------------------------------------------------------------
def restated_decode_step_rows(q, k_new, v_new, k_prefix, v_prefix, rows_b, rows_max, k_tail, v_tail, tail_rows, scaling):
    """_kvc.decode_step_rows restated in fp32: the step's rows are appended to the tail in place; batch row b attends to prefix rows
    [0, min(max(rows_b[b], 0), rows_max)) of each of its heads and to its KV head's tail rows [0, tail_rows + i + 1) for token i."""
    b, hq, t, D = q.shape
    g = hq // k_new.shape[1]
    k_tail[:, :, tail_rows:tail_rows + t] = k_new
    v_tail[:, :, tail_rows:tail_rows + t] = v_new
    out = torch.empty(b, t, hq, D, dtype=q.dtype)
    for r in range(b):
        P = min(max(int(rows_b[r]), 0), rows_max)
        for i in range(t):
            T = tail_rows + i + 1
            K = torch.cat([k_prefix[r, :, :P], k_tail[r, :, :T].repeat_interleave(g, 0)], 1).float()
            V = torch.cat([v_prefix[r, :, :P], v_tail[r, :, :T].repeat_interleave(g, 0)], 1).float()
            w = torch.softmax(torch.einsum("hd,hrd->hr", q[r, :, i].float(), K) * scaling, -1)
            out[r, i] = torch.einsum("hr,hrd->hd", w, V).to(q.dtype)
    return out


@pytest.fixture()
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(_kvc, "compress", oracle_compress)
    monkeypatch.setattr(_kvc, "compress_batch", oracle_compress_batch)
    monkeypatch.setattr(_kvc, "compress_merge", oracle_compress_merge)
    monkeypatch.setattr(_kvc, "l2norm_compress", oracle_l2norm_compress)
    monkeypatch.setattr(_kvc, "decode_step", oracle_decode_step)
    monkeypatch.setattr(_kvc, "decode_step_rows", restated_decode_step_rows, raising=False)
    yield


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bf(g, *sh):
    return torch.randn(*sh, generator=g).to(torch.bfloat16)


# ---- 1. geometry ---------------------------------------------------------------------------------------------------------------
def _masks(visible):
    """The three masks a prefill can see for per-row `visible` patterns [b, L] (bool): sdpa's 4-D bool, eager's 4-D additive,
    the tokenizer's 2-D."""
    b, L = visible.shape
    causal = torch.tril(torch.ones(L, L, dtype=torch.bool))
    m4 = causal[None, None] & visible[:, None, None, :]
    add = torch.zeros(b, 1, L, L).masked_fill(~m4, torch.finfo(torch.float32).min)
    return m4, add, visible.long()


def test_row_starts_from_bool_additive_and_2d_masks():
    from kvcache_factory_amd import pyramidkv_utils as pu
    L, starts = 12, (5, 0, 11, 3)
    vis = torch.stack([torch.arange(L) >= s for s in starts])
    for m in _masks(vis):
        assert pu.row_starts(m, 4, L) == starts
    for m in _masks(torch.ones(3, L, dtype=torch.bool)):                  # nothing padded
        assert pu.row_starts(m, 3, L) == (0, 0, 0)


@pytest.mark.parametrize("pattern,msg", [
    ([1, 1, 1, 1, 0, 0], "LEFT-padded"),                                  # right padding
    ([0, 1, 1, 0, 1, 1], "LEFT-padded"),                                  # a hole
    ([0, 0, 0, 0, 0, 0], "no visible column"),                            # nothing visible
])
def test_row_starts_refuses_what_is_not_left_padding(pattern, msg):
    from kvcache_factory_amd import pyramidkv_utils as pu
    vis = torch.tensor([[0, 0, 1, 1, 1, 1], pattern], dtype=torch.bool)
    for m in _masks(vis):
        with pytest.raises(ValueError, match=msg) as e:
            pu.row_starts(m, 2, 6)
        assert "row 1" in str(e.value)


def test_geometry_is_kept_per_prompt_and_bsz_1_never_looks(monkeypatch):
    from kvcache_factory_amd import pyramidkv_utils as pu

    class Untouchable:                                                    # any use of the mask would raise
        def __getattr__(self, name):
            raise AssertionError(f"the mask was inspected ({name})")
    pb = pu.PrefillBatch()
    assert pb.geometry(Untouchable(), 1, 9, fresh=True) is None
    assert pb.geometry(None, 3, 9, fresh=True) is None                    # no mask: nothing is padded
    calls = []
    real = pu.row_starts
    monkeypatch.setattr(pu, "row_starts", lambda *a: calls.append(a) or real(*a))
    vis = torch.stack([torch.arange(9) >= s for s in (4, 0)])
    m4 = _masks(vis)[0]
    assert pb.geometry(m4, 2, 9, fresh=True) == (4, 0)
    for _ in range(3):                                                    # the prompt's other layers: no second read
        assert pb.geometry(m4, 2, 9, fresh=False) == (4, 0)
    assert len(calls) == 1
    assert pb.geometry(_masks(torch.ones(2, 9, dtype=torch.bool))[0], 2, 9, fresh=True) is None     # a new prompt: derived anew
    assert len(calls) == 2


# ---- 2. per-row equivalence at the cluster level -----------------------------------------------------------------------------------
HQ, HKV, D, CAP, W = 4, 2, 64, 32, 8
LENS = (20, 40, 70)                   # below the cap; PyramidKV's middle branch (cap <= L < 2 (cap - W)); above 2 (cap - W)


def _cluster(name, layer_idx=0, n_layers=4, cap=CAP):
    from kvcache_factory_amd import pyramidkv_utils as pu
    kw = dict(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool")
    if name == "snapkv":
        return pu.SnapKVCluster(**kw)
    if name == "pyramidkv":
        return pu.PyramidKVCluster(num_hidden_layers=n_layers, layer_idx=layer_idx, **kw)
    if name == "streamingllm":
        return pu.StreamingLLMKVCluster(**kw)
    if name == "h2o":
        return pu.H2OKVCluster(**kw)
    return pu.L2NormCluster(max_capacity_prompt=cap, layer_idx=layer_idx, skip_layers=[1])


def _padded_batch(g, lens):
    """Per-row q / k / v and the left-padded batch built from them; the pad columns hold random garbage, not zeros."""
    L = max(lens)
    rows = [(_bf(g, 1, HQ, n, D), _bf(g, 1, HKV, n, D), _bf(g, 1, HKV, n, D)) for n in lens]
    Q, K, V = _bf(g, len(lens), HQ, L, D) * 30, _bf(g, len(lens), HKV, L, D) * 30, _bf(g, len(lens), HKV, L, D) * 30
    for b, (q, k, v) in enumerate(rows):
        Q[b, :, L - lens[b]:], K[b, :, L - lens[b]:], V[b, :, L - lens[b]:] = q[0], k[0], v[0]
    return rows, Q, K, V, tuple(L - n for n in lens)


def _alone(cluster, q, k, v):
    """What the prompt keeps when it is run alone (pass-through rows cached repeat_kv-expanded, as the patched forward does)."""
    kc, vc = cluster.update_kv(k, q, v, None, HQ // HKV)
    if kc is k:
        kc, vc = k.repeat_interleave(HQ // HKV, 1), v.repeat_interleave(HQ // HKV, 1)
    return kc, vc


def _check_rows(layer, cluster, rows):
    lengths = layer.row_lengths().tolist()
    for b, (q, k, v) in enumerate(rows):
        kc, vc = _alone(cluster, q, k, v)
        assert lengths[b] == kc.shape[2], (b, lengths, kc.shape)
        assert torch.equal(_bits(layer._kbuf[b:b + 1, :, :lengths[b]]), _bits(kc)), b
        assert torch.equal(_bits(layer._vbuf[b:b + 1, :, :lengths[b]]), _bits(vc)), b
    return lengths


@pytest.mark.parametrize("parked", [True, False], ids=["prefill_batch", "direct"])
@pytest.mark.parametrize("method,layer_idx", [("snapkv", 0), ("pyramidkv", 0), ("pyramidkv", 3), ("streamingllm", 0), ("h2o", 0),
                                              ("l2norm", 0), ("l2norm", 1)])
def test_each_row_keeps_what_the_prompt_keeps_alone(cpu_kernels, method, layer_idx, parked):
    from kvcache_factory_amd import pyramidkv_utils as pu
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    g = torch.Generator().manual_seed(17 + layer_idx)
    rows, Q, K, V, starts = _padded_batch(g, LENS)
    cluster, layer = _cluster(method, layer_idx), CompressedDynamicLayer()
    pending = pu.PrefillBatch() if parked else None
    got = pu.prefill_rows(cluster, layer, K, Q, V, starts, HQ // HKV, pending)
    if parked:
        pending.flush(overlap=True)
        pending.settle()
    lengths = _check_rows(layer, cluster, rows)
    assert got == lengths and lengths[0] == LENS[0]                        # the short prompt is passed through: its own length
    if method == "pyramidkv":
        assert lengths[1] == CAP and lengths[2] == _kvc.pyramid_k(CAP, W, LENS[2], layer_idx, 4) + W
    elif method == "l2norm" and layer_idx == 1:
        assert lengths == list(LENS)                                       # a skipped layer keeps everything
    else:
        assert lengths[1:] == [CAP, CAP]
    assert layer.has_holes() and layer.get_seq_length() == max(LENS) and layer._stored == max(lengths)
    assert layer.get_mask_sizes(1) == (max(lengths) + 1, 0)
    assert layer.keys.shape == (3, HQ, max(lengths), D)                    # the padded view


def test_rows_of_one_length_share_one_batched_call(cpu_kernels, monkeypatch):
    """Two layers x (two rows of 40, one of 70): the parked rows are grouped by length — one call with four items, one with two."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    seen = []

    def spy(method, qs, ks, vs, *a, **kw):
        seen.append((len(ks), ks[0].shape[0], ks[0].shape[2]))
        return oracle_compress_batch(method, qs, ks, vs, *a, **kw)
    monkeypatch.setattr(_kvc, "compress_batch", spy)
    g = torch.Generator().manual_seed(3)
    pending, layers, batches = pu.PrefillBatch(), [], []
    for _ in range(2):
        rows, Q, K, V, starts = _padded_batch(g, (40, 70, 40))
        layer = CompressedDynamicLayer()
        pu.prefill_rows(_cluster("snapkv"), layer, K, Q, V, starts, HQ // HKV, pending)
        assert pending.holds(layer)
        layers.append(layer), batches.append(rows)
    pending.flush(overlap=True)
    assert sorted(seen) == [(2, 1, 70), (4, 1, 40)]
    for layer, rows in zip(layers, batches):
        assert _check_rows(layer, _cluster("snapkv"), rows) == [CAP] * 3 and not layer.has_holes()


# ---- 4. the layer with unequal rows --------------------------------------------------------------------------------------------
def _layer_with_rows(g, rows, cls=None, **kw):
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    layer = (cls or CompressedDynamicLayer)(**kw)
    kb, vb = layer.reserve_rows(len(rows), HQ, rows, D, torch.bfloat16, torch.device("cpu"), 16)
    kb.copy_(_bf(g, *kb.shape)), vb.copy_(_bf(g, *vb.shape))
    layer.prefill_rows(rows, 50)
    assert all(not kb[b, :, n:max(rows)].any() and not vb[b, :, n:max(rows)].any() for b, n in enumerate(rows))   # holes are zeroed
    for b, n in enumerate(rows):                                            # from here on whatever lies behind a row's last row is
        kb[b, :, n:], vb[b, :, n:] = float("nan"), float("nan")            # poison: the per-row step must never read it
    return layer


def test_own_mask_hides_exactly_the_holes_and_both_forms_agree(cpu_kernels):
    g = torch.Generator().manual_seed(23)
    rows = [9, 3, 14, 14, 1]
    split, shaped = _layer_with_rows(g, rows), _layer_with_rows(torch.Generator().manual_seed(23), rows)
    assert split.has_holes() and split.row_lengths().tolist() == rows and split.row_lengths().dtype == torch.int32
    for step, t in enumerate((1, 3, 1)):
        q, k, v = _bf(g, 5, HQ, t, D), _bf(g, 5, HKV, t, D), _bf(g, 5, HKV, t, D)
        out = split.decode_attend(q, k, v, D ** -0.5)                       # SPLIT: the per-row step
        K, V = shaped.update(k.repeat_interleave(2, 1), v.repeat_interleave(2, 1))       # EXPANDED: appended from row 14 on
        total = K.shape[2]
        assert total == 14 + sum((1, 3, 1)[:step + 1]) and shaped.get_mask_sizes(1) == (total + 1, 0)
        m = shaped.decode_mask(t, torch.float32)
        assert m.shape == (5, 1, t, total)
        col = torch.arange(total)
        for b, n in enumerate(rows):
            for i in range(t):
                hidden = ((col >= n) & (col < 14)) | (col > total - t + i)
                assert torch.equal(m[b, 0, i] != 0, hidden) and set(m[b, 0, i].unique().tolist()) <= {0.0, torch.finfo(torch.float32).min}
        w = torch.softmax(q.float() @ K.float().nan_to_num(0.0).transpose(2, 3) * D ** -0.5 + m, -1)
        ref = (w @ V.float().nan_to_num(0.0)).transpose(1, 2)
        assert not torch.isnan(out.float()).any()
        assert float((out.float() - ref).abs().max()) <= 2.0 ** -7 * max(1.0, float(ref.abs().max()))
    assert split.get_seq_length() == shaped.get_seq_length() == 55
    assert split.keys.shape == shaped.keys.shape                            # padded views: prefix bound + decoded rows
    split._expand()                                                         # SPLIT -> EXPANDED keeps the holes and the lengths
    assert split.row_lengths().tolist() == rows and split._pmax == 14 and split._stored == 19
    assert torch.equal(split.decode_mask(1, torch.float32), shaped.decode_mask(1, torch.float32))


def test_batch_operations_carry_the_row_lengths(cpu_kernels):
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    assert "_rows" in CompressedDynamicLayer._batch_tensors
    g = torch.Generator().manual_seed(29)
    rows = [9, 3, 14]
    layer = _layer_with_rows(g, rows)
    before = _bits(layer._kbuf).clone()
    beam = torch.tensor([2, 0, 0])
    layer.reorder_cache(beam)
    assert layer.row_lengths().tolist() == [14, 9, 9] and torch.equal(_bits(layer._kbuf), before[beam])
    layer.batch_repeat_interleave(2)
    assert layer.row_lengths().tolist() == [14, 14, 9, 9, 9, 9] and layer._kbuf.shape[0] == 6
    layer.batch_select_indices(torch.tensor([1, 4]))
    assert layer.row_lengths().tolist() == [14, 9] and layer._kbuf.shape[0] == 2
    q, k, v = _bf(g, 2, HQ, 1, D), _bf(g, 2, HKV, 1, D), _bf(g, 2, HKV, 1, D)
    out = layer.decode_attend(q, k, v, D ** -0.5)                            # rows and buffers still belong together: no poison read
    assert not torch.isnan(out.float()).any()


def test_uniform_rows_leave_the_layer_as_it_is_today(cpu_kernels):
    g = torch.Generator().manual_seed(31)
    layer = _layer_with_rows(g, [12, 12, 12])
    assert not layer.has_holes() and layer._rows is None and layer._stored == 12
    assert layer.row_lengths().tolist() == [12, 12, 12]


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def _config(layers=2, attn="sdpa"):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                       head_dim=64, vocab_size=128, max_position_embeddings=2048, attn_implementation=attn)


class _Patched:
    """A tiny bf16 Llama with the attention forwards of `method` (restored on exit)."""

    def __init__(self, method, cap=16, W=4, merge=None, attn="sdpa"):
        self.method, self.knobs, self.attn = method, dict(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool",
                                                          merge=merge), attn

    def __enter__(self):
        from transformers import LlamaForCausalLM
        from kvcache_factory_amd import monkeypatch as mp
        torch.manual_seed(0)
        model = LlamaForCausalLM(_config(attn=self.attn)).eval().to(torch.bfloat16)
        mp.replace_llama(self.method)
        for layer in model.model.layers:
            for name, val in self.knobs.items():
                setattr(layer.self_attn.config, name, val)
        return model

    def __exit__(self, *exc):
        from kvcache_factory_amd import monkeypatch as mp
        mp.replace_llama("fullkv")


def _prompts(lens, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 128, (1, n), generator=g) for n in lens]


def _pad_left(prompts):
    L = max(p.shape[1] for p in prompts)
    ids = torch.cat([torch.cat([torch.zeros(1, L - p.shape[1], dtype=torch.long), p], 1) for p in prompts])
    mask = torch.cat([torch.cat([torch.zeros(1, L - p.shape[1], dtype=torch.long), torch.ones_like(p)], 1) for p in prompts])
    return ids, mask


def _prefill(model, prompts, cache):
    ids, mask = _pad_left(prompts)
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        return model(ids, attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True).logits, mask


@pytest.mark.parametrize("method,merge,name", [("snapkv", "pivot", "merge='pivot'"), ("cam", None, "CAM"), ("think", None, "ThinK")])
def test_methods_without_a_per_row_form_refuse_a_padded_batch(cpu_kernels, method, merge, name):
    from transformers import DynamicCache
    cache = DynamicCache()
    with _Patched(method, merge=merge) as model:
        with pytest.raises(NotImplementedError, match=name):
            _prefill(model, _prompts((27, 40)), cache)
    assert all(layer.get_seq_length() == 0 for layer in cache.layers)


def _special_caches():
    from kvcache_factory_amd import DecodeCompressedCache, KVQuantCompressedCache, QuantizedCompressedCache
    return [lambda c: DecodeCompressedCache(c, interval=8), lambda c: QuantizedCompressedCache(c, nbits=4),
            lambda c: KVQuantCompressedCache(c, nbits=4)]


@pytest.mark.parametrize("make", _special_caches(), ids=["decode_compressed", "quantized", "kvquant"])
def test_special_caches_refuse_unequal_rows_before_anything_is_stored(cpu_kernels, make):
    cache = make(_config())
    with _Patched("snapkv") as model:
        with pytest.raises(NotImplementedError, match=r"\[13, 16\] rows per prompt") as e:
            _prefill(model, _prompts((13, 40)), cache)                       # 13 < cap: passed through; 40 -> 16
    assert type(cache.layers[0]).__name__ in str(e.value)
    for layer in cache.layers:
        assert layer.get_seq_length() == 0 and layer._kbuf is None and layer.stored_length() == 0


@pytest.mark.parametrize("make", _special_caches(), ids=["decode_compressed", "quantized", "kvquant"])
def test_special_caches_take_a_padded_batch_that_compresses_to_equal_rows(cpu_kernels, monkeypatch, make):
    """SnapKV with every prompt at or above the cap: every row keeps cap rows — what lands in the special cache's layers is, row by
    row, what the stand-in returns for that row's slice of the Q / K / V the prefill handed over."""
    from kvcache_factory_amd import pyramidkv_utils as pu
    seen = []
    real = pu.prefill_rows

    def spy(cluster, layer, K, Q, V, starts, groups, pending=None):
        seen.append((layer, K.clone(), Q.clone(), V.clone(), starts))
        return real(cluster, layer, K, Q, V, starts, groups, pending)
    monkeypatch.setattr(pu, "prefill_rows", spy)
    cache = make(_config())
    with _Patched("snapkv") as model:
        _prefill(model, _prompts((27, 40, 16)), cache)
    assert len(seen) == 2
    cl = pu.SnapKVCluster(window_size=4, max_capacity_prompt=16, kernel_size=7, pooling="maxpool")
    for layer, K, Q, V, starts in seen:
        assert starts == (13, 0, 24) and layer.get_seq_length() == 40 and layer.stored_length() == 16 and not layer.has_holes()
        for b, s in enumerate(starts):
            kc, vc = cl.update_kv(K[b:b + 1, :, s:], Q[b:b + 1, :, s:], V[b:b + 1, :, s:], None, 2)
            assert torch.equal(_bits(layer._kbuf[b:b + 1, :, :16]), _bits(kc)) and torch.equal(_bits(layer._vbuf[b:b + 1, :, :16]), _bits(vc))


# ---- 3. model level: a padded batch against the same prompts alone ------------------------------------------------------------------
STEPS = 4


def _solo(model, prompt):
    """Greedy, STEPS decode steps: the logits of the prefill's last position and of every decode step, and the tokens chosen."""
    from transformers import DynamicCache
    cache, logits, tokens = DynamicCache(), [], []
    with torch.no_grad():
        out = model(prompt, past_key_values=cache, use_cache=True).logits[:, -1]
        for _ in range(STEPS):
            logits.append(out[0].float())
            tokens.append(int(out.argmax(-1)))
            out = model(torch.tensor([[tokens[-1]]]), past_key_values=cache, use_cache=True).logits[:, -1]
        logits.append(out[0].float())
    return logits, tokens


def _teacher_forced_batch(model, prompts, tokens, cache):
    """The padded batch, every row fed the tokens its solo run chose: logits [step][row] like _solo's."""
    logits, mask = _prefill(model, prompts, cache)
    out = [logits[:, -1].float()]
    lens = mask.sum(-1)
    for j in range(STEPS):
        mask = torch.cat([mask, torch.ones(len(prompts), 1, dtype=torch.long)], 1)
        step = torch.tensor([[tokens[b][j]] for b in range(len(prompts))])
        with torch.no_grad():
            out.append(model(step, attention_mask=mask, position_ids=(lens + j)[:, None], past_key_values=cache,
                             use_cache=True).logits[:, -1].float())
    return out


@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("method", ["snapkv", "pyramidkv"])
def test_padded_batch_decodes_like_the_prompts_alone(cpu_kernels, method, attn):
    """Two-layer bf16 Llama (4 query / 2 KV heads of 64), max_capacity_prompt 16, window 4, maxpool 7; prompts of 27 and 40 tokens,
    the first left-padded by 13.  Each prompt is generated alone (greedy, 4 decode steps); then the padded batch is driven with
    the tokens the solo runs chose.  For BOTH rows and EVERY one of the 4 decode steps (and the prefill's own logits) the batch's
    logits are within 3e-2 * max|logit| of the solo run's (the tolerance of test_decode_logits_vs_oracle_built_cache; the
    unpatched model with a stock DynamicCache differs by at most 0.005 * max|logit| between the two ways of running).
    Before per-row compression: steps 1-3 of the padded row differed by 1.00, 1.23 and 1.39 where the largest logit is 0.82-1.04."""
    from transformers import DynamicCache
    prompts = _prompts((27, 40))
    with _Patched(method, attn=attn) as model:
        solo = [_solo(model, p) for p in prompts]
        cache = DynamicCache()
        batch = _teacher_forced_batch(model, prompts, [s[1] for s in solo], cache)
    for b in range(2):
        for j in range(STEPS + 1):
            ref = solo[b][0][j]
            err, scale = float((batch[j][b] - ref).abs().max()), float(ref.abs().max())
            print(f"{method} {attn} row {b} step {j}: max |logit diff| {err:.4f}, max |logit| {scale:.4f}, allowed {3e-2 * scale:.4f}")
            assert err <= 3e-2 * scale, (method, b, j, err, scale)
    assert all(layer.get_seq_length() == 40 + STEPS for layer in cache.layers)
    if method == "snapkv":
        assert [layer.row_lengths().tolist() for layer in cache.layers] == [[16, 16]] * 2


def test_padded_batch_with_a_passed_through_row_decodes_like_the_prompts_alone(cpu_kernels):
    """Rows that keep DIFFERENT numbers of rows (13 < cap is passed through, 40 -> 16): the reference-shaped form with the layer's own
    mask over the holes, same bound as above."""
    from transformers import DynamicCache
    prompts = _prompts((13, 40, 27), seed=5)
    with _Patched("snapkv") as model:
        solo = [_solo(model, p) for p in prompts]
        cache = DynamicCache()
        batch = _teacher_forced_batch(model, prompts, [s[1] for s in solo], cache)
    for b in range(3):
        for j in range(STEPS + 1):
            ref = solo[b][0][j]
            assert float((batch[j][b] - ref).abs().max()) <= 3e-2 * float(ref.abs().max()), (b, j)
    assert [layer.row_lengths().tolist() for layer in cache.layers] == [[13, 16, 16]] * 2 and cache.layers[0].has_holes()


# ---- 6. C-ABI ----------------------------------------------------------------------------------------------------------------------
def _dp(kvc, **kw):
    p = kvc.DecodeParams()
    base = dict(dtype=kvc.BF16, bsz=8, n_q_heads=32, n_kv_heads=8, head_dim=128, prefix_rows=2056, tail_rows=256, new_rows=1,
                scaling=128 ** -0.5, q_stride_b=32 * 128, q_stride_h=128, q_stride_l=128, new_stride_b=8 * 128, new_stride_h=128,
                new_stride_l=128, prefix_stride_b=32 * 2312 * 128, prefix_stride_h=2312 * 128, tail_stride_b=8 * 320 * 128,
                tail_stride_h=320 * 128, out_stride_b=32 * 128, out_stride_h=128, out_stride_l=32 * 128)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def test_decode_step_rows_is_exported_and_sizes_its_workspace(kvc):
    assert {"kvc_decode_step_rows", "kvc_decode_rows_workspace_bytes"} <= set(kvc.EXPORTS)
    L = kvc.lib()
    assert L.kvc_version() == 5                                              # the ABI is additive
    n = L.kvc_decode_rows_workspace_bytes(ctypes.byref(_dp(kvc)))
    assert n > 0 and n % (130 * 4 * 8 * 32) == 0                             # whole (m, l, acc[128]) records per (row, head, split)
    assert L.kvc_decode_rows_workspace_bytes(ctypes.byref(_dp(kvc, prefix_rows=0, tail_rows=0))) == 0      # one split: none needed


BAD = [(dict(dtype=3), -1, "dtype"), (dict(dtype=-1), -1, "dtype"), (dict(bsz=0), -1, "bsz"), (dict(n_q_heads=0), -1, "head counts"),
       (dict(n_kv_heads=0), -1, "head counts"), (dict(n_kv_heads=5), -1, "head counts"), (dict(head_dim=96), -2, "head_dim"),
       (dict(prefix_rows=-1), -1, "row counts"), (dict(tail_rows=-1), -1, "row counts"), (dict(new_rows=0), -1, "row counts")]


@pytest.mark.parametrize("kw,code,msg", BAD, ids=[f"{list(b[0])[0]}={list(b[0].values())[0]}" for b in BAD])
def test_decode_step_rows_rejects_invalid_params_before_any_pointer(kvc, kw, code, msg):
    L = kvc.lib()
    a = ctypes.c_void_p(1 << 40)                                             # never dereferenced
    rc = L.kvc_decode_step_rows(ctypes.byref(_dp(kvc, **kw)), *([a] * 10), 1 << 20, None)
    assert rc == code and msg in L.kvc_last_error().decode(), (rc, L.kvc_last_error())
    assert L.kvc_decode_rows_workspace_bytes(ctypes.byref(_dp(kvc, **kw))) == 0


def test_decode_step_rows_rejects_null_and_misaligned_pointers(kvc):
    L = kvc.lib()
    a, odd, off4 = ctypes.c_void_p(1 << 40), ctypes.c_void_p((1 << 40) + 2), ctypes.c_void_p((1 << 40) + 8)
    p = _dp(kvc)
    assert L.kvc_decode_step_rows(None, *([a] * 10), 0, None) == -1 and b"NULL" in L.kvc_last_error()
    assert L.kvc_decode_step_rows(ctypes.byref(p), *([None] * 10), 0, None) == -1
    assert L.kvc_decode_step_rows(ctypes.byref(p), None, *([a] * 9), 0, None) == -1 and b"prefix_rows_b" in L.kvc_last_error()
    assert L.kvc_decode_step_rows(ctypes.byref(p), odd, *([a] * 9), 0, None) == -4 and b"prefix_rows_b" in L.kvc_last_error()
    for hole in range(1, 9):                                                 # q, k_new, v_new, k_prefix, v_prefix, k_tail, v_tail, out
        args = [a] * 10
        args[hole] = None
        assert L.kvc_decode_step_rows(ctypes.byref(p), *args, 0, None) == -1 and b"non-NULL" in L.kvc_last_error(), hole
    for where in (1, 4, 6, 9):                                               # q, k_prefix, k_tail, workspace
        args = [a] * 10
        args[where] = off4
        assert L.kvc_decode_step_rows(ctypes.byref(p), *args, 1 << 20, None) == -4 and b"aligned" in L.kvc_last_error(), where
    assert L.kvc_decode_step_rows(ctypes.byref(_dp(kvc, prefix_stride_h=2312 * 128 + 4)), *([a] * 10), 0, None) == -4
