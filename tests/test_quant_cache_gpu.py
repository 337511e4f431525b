"""The quantized decode cache on the MI355X: quantize kernels bit for bit against the numpy restatement (tests/quant_ref.py),
de-quantization within 1 ulp, kvc_decode_step_quant against fp32 attention over the restated de-quantized cache, the model
end to end (fused step vs the reference-shaped path, 8-bit vs the unquantized cache, fullkv), memory, beam search."""
import numpy as np
import pytest
import torch

import quant_ref as Q

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 1e-5}


def _src(g, dtype, b, h, rows, spare, D, G, dev):
    """[b, h, rows, D] view of a buffer with spare rows per head; one constant key group column and one constant value group."""
    x = torch.randn(b, h, rows + spare, D, generator=g) * 3
    x[:, :, :G, 3] = 1.5                                                     # key group 0, channel 3: scale 0
    x[:, :, G + 7, :G] = -2.0                                                # value row G + 7, channel group 0: scale 0
    x = x.to(dtype).to(dev)
    return x[:, :, :rows]


@pytest.mark.parametrize("nbits,G,dtype,D", [(nb, G, dt, D) for nb in (2, 4, 8) for G in (32, 64, 128)
                                               for dt in (torch.bfloat16, torch.float16, torch.float32) for D in (64, 128) if G <= D])
def test_quantize_rows_bit_identical(kvc, gpu_device, nbits, G, dtype, D):
    g = torch.Generator().manual_seed(nbits * 1000 + G + D)
    b, h, rows, row0 = 2, 3, 2 * G + 5, G                                    # partial last key group; written behind a first group
    x = _src(g, dtype, b, h, rows, 9, D, G, gpu_device)
    assert x.stride(1) == (rows + 9) * D
    kc, vc, km, vm = kvc.quant_buffers(b, h, row0 + rows + 3, D, nbits, G, gpu_device)
    kvc.quantize_rows(x, kc, km, row0, kvc.QUANT_KEYS, nbits, G)
    kvc.quantize_rows(x, vc, vm, row0, kvc.QUANT_VALUES, nbits, G)
    torch.cuda.synchronize()
    xf = x.float().cpu().numpy()
    for mode, codes, meta in ((Q.KEYS, kc, km), (Q.VALUES, vc, vm)):
        c, s, z = Q.quantize(xf, mode, nbits, G)
        got_c = codes[:, :, row0:row0 + rows].cpu().numpy()
        assert np.array_equal(got_c, Q.pack(c, nbits)), mode
        m = meta.cpu().numpy()
        m = m[:, :, 1:1 + s.shape[2]] if mode == Q.KEYS else m[:, :, row0:row0 + rows]
        assert np.array_equal(m.view(np.int32), Q.meta_array(s, z, mode).view(np.int32)), mode
        if mode == Q.KEYS:
            assert (s[:, :, 0, 3] == 0).all() and (c[:, :, :G, 3] == 0).all()
        else:
            assert (s[:, :, G + 7, 0] == 0).all() and (c[:, :, G + 7, :G] == 0).all()
    # de-quantization: within 1 ulp of fp32 of the restatement (which rounds through float64)
    for mode, codes, meta in ((Q.KEYS, kc, km), (Q.VALUES, vc, vm)):
        for odt in (torch.float32, dtype):
            got = kvc.dequantize_rows(codes, meta, row0, rows, mode, nbits, G, odt).float().cpu().numpy()
            c, s, z = Q.quantize(xf, mode, nbits, G)
            ref = Q.dequantize(c, s, z, mode, G)
            if odt == torch.float32:
                assert (np.abs(got - ref) <= np.spacing(np.abs(ref))).all(), mode
            else:
                refd = torch.from_numpy(ref).to(odt).float().numpy()            # 1 ulp of the 16-bit type (+ its subnormal step)
                ulp = np.spacing(np.abs(refd)) * (2.0 ** 16 if odt == torch.bfloat16 else 2.0 ** 13) + 2.0 ** -24
                assert (np.abs(got - refd) <= ulp).all(), mode


def _segment(kvc, g, dtype, b, heads, rows, D, nbits, G, dev):
    k = (torch.randn(b, heads, rows, D, generator=g)).to(dtype).to(dev)
    v = (torch.randn(b, heads, rows, D, generator=g)).to(dtype).to(dev)
    bufs = kvc.quant_buffers(b, heads, rows + G, D, nbits, G, dev)
    kvc.quantize_rows(k, bufs[0], bufs[2], 0, kvc.QUANT_KEYS, nbits, G)
    kvc.quantize_rows(v, bufs[1], bufs[3], 0, kvc.QUANT_VALUES, nbits, G)
    rk = torch.from_numpy(Q.roundtrip(k, Q.KEYS, nbits, G)) if rows else torch.zeros(b, heads, 0, D)
    rv = torch.from_numpy(Q.roundtrip(v, Q.VALUES, nbits, G)) if rows else torch.zeros(b, heads, 0, D)
    return (*bufs, rows), rk, rv


@pytest.mark.parametrize("dtype,D,hq,hkv,P,Tq,res,t,nbits,G", [
    (torch.bfloat16, 128, 32, 8, 128, 0, 0, 1, 4, 64), (torch.bfloat16, 128, 32, 8, 128, 32, 5, 1, 2, 32),
    (torch.float16, 64, 8, 2, 40, 64, 5, 3, 8, 32), (torch.float32, 128, 4, 4, 70, 128, 9, 2, 4, 128),
    (torch.bfloat16, 128, 32, 8, 2056, 0, 100, 1, 4, 64), (torch.bfloat16, 128, 32, 8, 2056, 1024, 37, 2, 2, 64),
    (torch.bfloat16, 128, 32, 8, 2056, 1024, 20, 3, 8, 32), (torch.float16, 128, 8, 8, 4104, 0, 1, 1, 4, 128),
    (torch.bfloat16, 64, 4, 1, 63, 32, 1, 1, 2, 32), (torch.float32, 64, 8, 2, 257, 64, 63, 3, 8, 64)])
def test_decode_step_quant_vs_fp32_attention(kvc, gpu_device, dtype, D, hq, hkv, P, Tq, res, t, nbits, G):
    """Against fp32 attention over the de-quantized prefix (per query head), the de-quantized tail and the residual + new rows
    (per KV head, repeat_kv-expanded), causal among the step's tokens; tolerance as kvc_decode_step's test.  The residual must hold
    the appended rows byte for byte and its other rows untouched."""
    g = torch.Generator().manual_seed(P + Tq + res + nbits)
    R = max(128, G)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dtype).to(gpu_device)      # noqa: E731
    q, kn, vn = rn(1, hq, t, D), rn(1, hkv, t, D), rn(1, hkv, t, D)
    pre, pk, pv = _segment(kvc, g, dtype, 1, hq, P, D, nbits, G, gpu_device)
    tail, tk, tv = _segment(kvc, g, dtype, 1, hkv, Tq, D, nbits, G, gpu_device)
    kr, vr = rn(1, hkv, R + 8, D), rn(1, hkv, R + 8, D)
    kr0, vr0 = kr.clone(), vr.clone()
    out = kvc.decode_step_quant(q, kn, vn, pre, tail if Tq else None, kr, vr, res, D ** -0.5, nbits, G, R)
    assert out.shape == (1, t, hq, D)
    assert torch.equal(kr[:, :, res:res + t], kn) and torch.equal(vr[:, :, res:res + t], vn)
    assert torch.equal(kr[:, :, :res], kr0[:, :, :res]) and torch.equal(kr[:, :, res + t:], kr0[:, :, res + t:])
    grp = hq // hkv
    K = torch.cat([pk, tk.repeat_interleave(grp, 1), kr[:, :, :res + t].float().cpu().repeat_interleave(grp, 1)], 2)
    V = torch.cat([pv, tv.repeat_interleave(grp, 1), vr[:, :, :res + t].float().cpu().repeat_interleave(grp, 1)], 2)
    ref = Q.attention(q, K, V, D ** -0.5, causal_new=t)
    got = out.transpose(1, 2).float().cpu().numpy()
    assert float(np.abs(got - ref).max()) <= TOL[dtype] * max(1.0, float(np.abs(ref).max()))


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _model(dev):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=256, num_hidden_layers=3, num_attention_heads=32,
                      num_key_value_heads=8, head_dim=128, vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa")
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev).eval()


def _generate(model, ids, method, cache, n=70, **kw):
    from kvcache_factory_amd import monkeypatch as mp
    try:
        mp.replace_llama(method)
        if method != "fullkv":
            for layer in model.model.layers:
                for name, val in (("window_size", 8), ("max_capacity_prompt", 72), ("kernel_size", 7), ("pooling", "maxpool")):
                    setattr(layer.self_attn.config, name, val)
        with torch.no_grad():
            return model.generate(ids, max_new_tokens=n, min_new_tokens=n, do_sample=False, use_cache=True, return_dict_in_generate=True,
                                  output_scores=True, past_key_values=cache, **kw)
    finally:
        mp.replace_llama("fullkv")


def _compare_logits(a, b):
    """Step by step while both runs have seen the same tokens; a parting of the ways only at a near tie."""
    sa, sb = a.sequences[0, -len(a.scores):], b.sequences[0, -len(b.scores):]
    compared = 0
    for i, (x, y) in enumerate(zip(a.scores, b.scores)):
        x, y = x.float(), y.float()
        fin = torch.isfinite(y)                                              # min_new_tokens masks EOS with -inf in both runs
        assert torch.equal(fin, torch.isfinite(x))
        x, y = x[fin], y[fin]
        tol = 3e-2 * float(y.abs().max())
        assert float((x - y).abs().max()) <= tol, (i, float((x - y).abs().max()), tol)
        compared += 1
        if int(sa[i]) != int(sb[i]):
            yb = b.scores[i].float()
            assert abs(float(yb[0, sa[i]]) - float(yb[0, sb[i]])) <= tol, "tokens differ away from a tie"
            break
    return compared


@pytest.mark.parametrize("method", ["snapkv", "pyramidkv", "h2o"])
def test_model_fused_vs_reference_shaped_and_8bit_vs_unquantized(kvc, gpu_device, method, monkeypatch):
    """G = R = 32, 70 tokens (two flushes).  (a) The fused step against the DECODE_KERNEL = 0 path: the same quantized prompt byte for
    byte, the same lengths, layer 0's de-quantized cache identical while the tokens are, logits within 3e-2 of the largest.  8 bits:
    at 4 / 2 bits a last-bit difference of a decoded row (two bf16 attention kernels upstream) can move a group's min / max and with it
    whole groups of codes, which the logits then show beyond that bound.  (b) 8 bits against the unquantized compressed cache."""
    from kvcache_factory_amd import QuantizedCompressedCache, pyramidkv_utils as pu
    model = _model(gpu_device)
    ids = torch.randint(0, 256, (1, 500), generator=torch.Generator().manual_seed(5)).to(gpu_device)
    mk = lambda nb: QuantizedCompressedCache(model.config, nbits=nb, q_group_size=32, residual_length=32)   # noqa: E731
    fused = _generate(model, ids, method, mk(8))
    with monkeypatch.context() as m:
        m.setattr(pu, "DECODE_KERNEL", False)
        shaped = _generate(model, ids, method, mk(8))
    assert _compare_logits(fused, shaped) >= 2
    for la, lb in zip(fused.past_key_values.layers, shaped.past_key_values.layers):
        assert la._mode == "fused" and lb._mode == "shaped" and la._kbuf is None and lb._kbuf is None
        assert la.get_seq_length() == lb.get_seq_length() == 569
        assert la._trows == 64 and la._rrows == 5 and la.stored_length() == lb.stored_length()     # two flushes of 32
        for x, y in ((la._pkc, lb._pkc), (la._pvc, lb._pvc), (la._pkm, lb._pkm), (la._pvm, lb._pvm)):
            assert torch.equal(x, y)                                          # the same quantized prompt, byte for byte
    if torch.equal(fused.sequences, shaped.sequences):                       # layer 0's rows depend only on the tokens
        la, lb = fused.past_key_values.layers[0], shaped.past_key_values.layers[0]
        assert torch.equal(la.keys, lb.keys) and torch.equal(la.values, lb.values)
    plain = _generate(model, ids, method, None)                              # (b)
    assert _compare_logits(fused, plain) >= 2


def test_fullkv_with_the_quantized_cache(kvc, gpu_device):
    from kvcache_factory_amd import QuantizedCompressedCache
    model = _model(gpu_device)
    ids = torch.randint(0, 256, (1, 200), generator=torch.Generator().manual_seed(7)).to(gpu_device)
    out = _generate(model, ids, "fullkv", QuantizedCompressedCache(model.config, nbits=4, q_group_size=32, residual_length=32))
    assert out.sequences.shape == (1, 270)
    layer = out.past_key_values.layers[0]
    assert layer._prows == 200 and layer._trows == 64 and layer._rrows == 5 and layer.get_seq_length() == 269


def test_memory_after_the_first_decode_step(kvc, gpu_device):
    """P = 2056, D = 128, 4 bits, G = 64: 329 856 B per head instead of 1 052 672 (bf16), and no full-precision prompt left."""
    from kvcache_factory_amd.cache import CompressedDynamicLayer, QuantizedCompressedLayer
    g = torch.Generator().manual_seed(3)
    hq, hkv, P, D = 8, 2, 2056, 128
    layer = QuantizedCompressedLayer(nbits=4, q_group_size=64, residual_length=128)
    kb, vb = layer.reserve(1, hq, P + 256, D, torch.bfloat16, gpu_device)
    kb[:, :, :P].copy_(torch.randn(1, hq, P, D, generator=g).to(torch.bfloat16))
    vb[:, :, :P].copy_(torch.randn(1, hq, P, D, generator=g).to(torch.bfloat16))
    layer.prefill(kb[:, :, :P], vb[:, :, :P], 9000)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(torch.bfloat16).to(gpu_device)      # noqa: E731
    layer.decode_attend(rn(1, hq, 1, D), rn(1, hkv, 1, D), rn(1, hkv, 1, D), D ** -0.5)
    assert layer._kbuf is None and layer._vbuf is None
    held = {n: getattr(layer, n) for n in layer._batch_tensors if getattr(layer, n) is not None}
    assert set(held) == {"_pkc", "_pvc", "_pkm", "_pvm", "_rk", "_rv"}
    prompt = sum(t.numel() * t.element_size() for n, t in held.items() if n.startswith("_p"))
    assert prompt == 329856 * hq and prompt <= 0.32 * 1052672 * hq
    plain = CompressedDynamicLayer()
    plain.prefill(kb[:, :, :P], vb[:, :, :P], 9000)
    assert plain._kbuf.numel() * 2 * 2 >= 1052672 * hq


def test_beam_search_through_update(kvc, gpu_device):
    from kvcache_factory_amd import QuantizedCompressedCache
    model = _model(gpu_device)
    ids = torch.randint(0, 256, (1, 300), generator=torch.Generator().manual_seed(9)).to(gpu_device)
    cache = QuantizedCompressedCache(model.config, nbits=4, q_group_size=32, residual_length=32)
    out = _generate(model, ids, "snapkv", cache, n=40, num_beams=2)
    assert out.sequences.shape[1] == 340
    layer = out.past_key_values.layers[1]
    assert layer._mode == "shaped" and layer._trows == 32 and layer._pkc.shape[0] == 2
    names = [n for n in layer._batch_tensors if getattr(layer, n) is not None]
    before = {n: getattr(layer, n).clone() for n in names}
    kk = layer.keys
    layer.reorder_cache(torch.tensor([1, 0], device=gpu_device))
    for n in names:
        assert torch.equal(getattr(layer, n).view(torch.uint8), before[n][[1, 0]].view(torch.uint8)), n
    assert torch.equal(layer.keys, kk[[1, 0]])
