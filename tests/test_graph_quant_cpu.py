"""The quantized cache under graph replay, without a GPU: the device-counted quantized entry is declared, exported and checks its
arguments before any launch; its split plan depends on the bound alone (restated here) and so do the edges of the visible rows; the
flush-and-grow schedule against a brute-force simulation of QuantizedCompressedLayer's rule; the adapter the GPU file runs the
conformance harness through, driven here over a device-counted CPU stand-in; QuantizedDeviceLayer's and GraphDecoder(nbits=...)'s
host arithmetic and refusals on a tiny Llama with the kernel calls replaced by the numpy restatement (capture=False)."""
import ctypes
import math
import os
import re

import pytest
import torch

import decode_ref as R
import quant_ref as Q
from kvcache_factory_amd import _kvc
from test_batch_generation_cpu import _Patched, _config, _prompts, cpu_kernels  # noqa: F401
from test_decode_conformance_cpu import run_bound, run_needles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kvc_decode_quant_dev_workspace_bytes", "kvc_decode_step_quant_dev")


# ---- the plan and the edges, restated ---------------------------------------------------------------------------------------------
def quant_dev_split_plan(b, hq, t, P, qcap, rcap):
    """(splits, rows_per_split) of kvc_decode_step_quant_dev with a full workspace: the plan kvc_decode_step_quant makes for the BOUND
    P + qcap + rcap rows — a target of 1024 workgroups, at least 64 rows per split, at most 64 splits, whole multiples of 64 rows."""
    rows = P + qcap + rcap
    heads = b * hq * t
    s = max(1, min(-(-1024 // heads), -(-rows // 64), 64))
    if s == 1:
        return 1, rows
    rps = -(-(-(-rows // s)) // 64) * 64
    return -(-rows // rps), rps


def visible_edges(b, hq, t, P, qcap, rcap, G):
    """(Tq, Rr) pairs at which the LAST token's visible rows P + Tq + Rr + t sit one below, at and one above every split boundary of
    the bound's plan, for every whole-group tail length that reaches it, plus both ends of both ranges."""
    splits, rps = quant_dev_split_plan(b, hq, t, P, qcap, rcap)
    out = {(0, 0), (0, rcap - t), (qcap, 0), (qcap, rcap - t)}
    for Tq in range(0, qcap + 1, G):
        for s in range(1, splits):
            for vis in (s * rps - 1, s * rps, s * rps + 1):
                Rr = vis - P - Tq - t
                if 0 <= Rr <= rcap - t:
                    out.add((Tq, Rr))
    return sorted(out)


def test_issue_setup_gives_four_splits_of_64_rows_and_its_edges():
    assert quant_dev_split_plan(1, 8, 1, 40, 128, 64) == (4, 64) and 40 + 128 + 64 == 232
    assert quant_dev_split_plan(1, 8, 3, 40, 128, 64) == (4, 64)
    e1 = set(visible_edges(1, 8, 1, 40, 128, 64, 32))
    assert {(0, 0), (0, 22), (0, 23), (0, 24), (64, 22), (64, 23), (64, 24), (32, 54), (32, 55), (32, 56), (128, 22), (128, 23),
            (128, 24), (128, 63)} <= e1
    e3 = set(visible_edges(1, 8, 3, 40, 128, 64, 32))
    assert {(0, 0), (0, 20), (0, 21), (0, 22), (128, 61), (64, 21)} <= e3
    for b, hq, t, P, qcap, rcap in ((1, 8, 1, 40, 128, 64), (2, 4, 3, 100, 1088, 8), (1, 32, 1, 2056, 2048, 128), (1, 8, 5, 12, 0, 6)):
        assert quant_dev_split_plan(b, hq, t, P, qcap, rcap) == R.split_plan(b, hq, t, P + qcap + rcap)      # the project's own statement
        assert quant_dev_split_plan(b, hq, t, P, qcap, rcap)[1] % 64 == 0 or quant_dev_split_plan(b, hq, t, P, qcap, rcap)[0] == 1


# ---- 1. the entry: declared, exported, checked before any pointer ---------------------------------------------------------------------
def test_header_declares_and_binding_exports_the_entry(kvc):
    header = open(os.path.join(ROOT, "include", "kvc.h")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header) and name in kvc.EXPORTS and hasattr(kvc.lib(), name)
    assert int(re.search(r"#define\s+KVC_VERSION\s+(\d+)", header).group(1)) == kvc.lib().kvc_version() == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in NEW)


def _qp(kvc, **kw):
    p = kvc.DecodeQuantParams()
    d = dict(dtype=kvc.BF16, bsz=1, n_q_heads=8, n_kv_heads=2, head_dim=128, nbits=4, group_size=32, residual_length=64, res_rows=0,
             res_capacity=64, new_rows=1, scaling=0.1, q_stride_b=1024, q_stride_h=128, q_stride_l=128, new_stride_b=256,
             new_stride_h=128, new_stride_l=128, res_stride_b=2 * 64 * 128, res_stride_h=64 * 128, out_stride_b=1024, out_stride_h=128,
             out_stride_l=1024)
    d.update(kw)
    for k, v in d.items():
        setattr(p, k, v)
    return p


def _seg(kvc, heads, rows, capacity, D=128, nbits=4, G=32, ptr=0):
    s = kvc.QuantSeg()
    cb = D * nbits // 8
    s.k_codes = s.v_codes = s.k_meta = s.v_meta = ptr
    s.rows, s.capacity = rows, capacity
    s.code_stride_h, s.code_stride_b = capacity * cb, heads * capacity * cb
    s.k_meta_stride_h = -(-capacity // G) * 2 * D
    s.k_meta_stride_b = heads * s.k_meta_stride_h
    s.v_meta_stride_h = capacity * (D // G) * 2
    s.v_meta_stride_b = heads * s.v_meta_stride_h
    return s


def _call(kvc, p, pre, qt, words=(0x1000, 0x1004), ptrs=None, ws=(None, 0)):
    ptrs = [0x10000 + 0x1000 * k for k in range(6)] if ptrs is None else ptrs
    return kvc.lib().kvc_decode_step_quant_dev(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(qt), words[0], words[1], *ptrs,
                                               ws[0], ws[1], None)


@pytest.mark.parametrize("kw,qcap,code,msg", [
    (dict(res_capacity=0), 128, _kvc.ERR_INVALID, "res_capacity"),
    (dict(new_rows=3, res_capacity=2, res_stride_h=2 * 128, res_stride_b=4 * 128), 128, _kvc.ERR_INVALID, "res_capacity"),
    (dict(), 100, _kvc.ERR_INVALID, "multiple of group_size"),
    (dict(nbits=3), 128, _kvc.ERR_INVALID, "nbits"),
    (dict(group_size=48), 128, _kvc.ERR_UNSUPPORTED, "group_size"),
    (dict(residual_length=40), 128, _kvc.ERR_INVALID, "residual_length"),
    (dict(head_dim=96), 128, _kvc.ERR_UNSUPPORTED, "head_dim"),
    (dict(n_kv_heads=3), 128, _kvc.ERR_INVALID, "head counts"),
    (dict(new_rows=0), 128, _kvc.ERR_INVALID, "new_rows"),
    (dict(res_stride_h=63 * 128), 128, _kvc.ERR_INVALID, "residual strides"),
])
def test_entry_rejects_invalid_params_before_any_pointer(kvc, kw, qcap, code, msg):
    """Every pointer handed over is a made-up address: a check that came after a pointer's first use would fault instead."""
    p = _qp(kvc, **kw)
    pre, qt = _seg(kvc, 8, 40, 40, ptr=0x100000), _seg(kvc, 2, 0, qcap, ptr=0x200000)
    assert _call(kvc, p, pre, qt) == code and msg in kvc.lib().kvc_last_error().decode()
    assert kvc.lib().kvc_decode_quant_dev_workspace_bytes(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(qt)) == 0


def test_entry_rejects_null_and_misaligned_pointers(kvc):
    p = _qp(kvc)
    pre, qt = _seg(kvc, 8, 40, 40, ptr=0x100000), _seg(kvc, 2, 77, 128, ptr=0x200000)     # qt.rows is ignored: 77 is no error
    err = lambda: kvc.lib().kvc_last_error().decode()                       # noqa: E731
    for words in ((None, 0x1004), (0x1000, None)):
        assert _call(kvc, p, pre, qt, words) == kvc.ERR_INVALID and "NULL" in err()
    assert _call(kvc, p, pre, qt, (0x1002, 0x1004)) == kvc.ERR_ALIGNMENT
    good = [0x10000 + 0x1000 * k for k in range(6)]
    for k in range(6):
        assert _call(kvc, p, pre, qt, ptrs=[None if j == k else x for j, x in enumerate(good)]) == kvc.ERR_INVALID
        assert _call(kvc, p, pre, qt, ptrs=[x + 8 if j == k else x for j, x in enumerate(good)]) == kvc.ERR_ALIGNMENT
    assert _call(kvc, p, pre, qt, ws=(0x300008, 1 << 20)) == kvc.ERR_ALIGNMENT
    assert _call(kvc, p, pre, _seg(kvc, 2, 0, 128, ptr=None)) == kvc.ERR_INVALID and "quantized tail" in err()
    assert _call(kvc, p, _seg(kvc, 8, 40, 40, ptr=None), qt) == kvc.ERR_INVALID and "prefix" in err()
    assert kvc.lib().kvc_decode_step_quant_dev(None, ctypes.byref(pre), ctypes.byref(qt), 0x1000, 0x1004, *good, None, 0, None) == kvc.ERR_INVALID
    assert kvc.lib().kvc_decode_step_quant_dev(ctypes.byref(p), ctypes.byref(pre), None, 0x1000, 0x1004, *good, None, 0, None) == kvc.ERR_INVALID


@pytest.mark.parametrize("b,hq,t,D,P,qcap,rcap", [(1, 8, 1, 128, 40, 128, 64), (1, 8, 3, 64, 40, 128, 64), (2, 4, 5, 128, 300, 1088, 8),
                                                  (1, 32, 1, 128, 2056, 2048, 128), (1, 8, 1, 64, 12, 0, 8), (1, 4, 1, 128, 20, 32, 32)])
def test_workspace_and_plan_follow_the_bound_only(kvc, b, hq, t, D, P, qcap, rcap):
    """The workspace holds (m, l, acc[D]) per (b, h, token, split) for the splits the bound asks for before they are rounded to whole
    multiples of 64 rows (never fewer than the plan uses) — whatever the two ignored lengths say."""
    G = 32
    sizes = set()
    for rows, res_rows in ((0, 0), (qcap, 0), (0, 5), (999999, -3)):
        p = _qp(kvc, bsz=b, n_q_heads=hq, n_kv_heads=hq // 2, head_dim=D, group_size=G, residual_length=max(64, rcap // G * G), res_rows=res_rows,
                res_capacity=rcap, new_rows=t, res_stride_h=rcap * D, res_stride_b=hq // 2 * rcap * D)
        pre, qt = _seg(kvc, hq, P, P, D, 4, G, ptr=0x100000), _seg(kvc, hq // 2, rows, qcap, D, 4, G, ptr=0x200000)
        sizes.add(kvc.lib().kvc_decode_quant_dev_workspace_bytes(ctypes.byref(p), ctypes.byref(pre), ctypes.byref(qt)))
        assert kvc.lib().kvc_last_error().decode() == ""
    raw = max(1, min(-(-1024 // (b * hq * t)), -(-(P + qcap + rcap) // 64), 64))
    assert raw >= quant_dev_split_plan(b, hq, t, P, qcap, rcap)[0]
    assert sizes == {0 if raw == 1 else b * hq * t * raw * (D + 2) * 4}


# ---- 2. the schedule ----------------------------------------------------------------------------------------------------------------
def _brute_schedule(R, G, capacity, steps):
    """QuantizedCompressedLayer's rule, step by step (decode_attend / _flush: once the residual holds >= R rows its oldest
    floor(rows / G) * G rows go onto the tail, the rest move to the front), on a tail that starts with `capacity` rows and doubles
    when the rows do not fit; a decoder captures before its first step and again before the first step after a doubling."""
    rrows = trows = 0
    flushes, tails, grows, captures, graph = [], [], 0, 0, False
    for step in range(1, steps + 1):
        if not graph:
            graph, captures = True, captures + 1
        rrows += 1
        if rrows >= R:
            n = rrows // G * G
            if trows + n > capacity:
                while trows + n > capacity:
                    capacity *= 2
                grows, graph = grows + 1, False
            trows, rrows = trows + n, rrows - n
            flushes.append(step)
            tails.append(trows)
    return flushes, tails, grows, captures


@pytest.mark.parametrize("R,G,capacity", [(64, 32, 64), (64, 64, 128), (128, 64, 128), (128, 32, 1024), (32, 32, 32), (256, 128, 256),
                                          (96, 32, 96), (64, 32, 192)])
def test_schedule_is_the_quantized_layers_rule(R, G, capacity):
    from kvcache_factory_amd.cache import quant_flush, quant_schedule
    got = quant_schedule(R, capacity, 1000)
    assert got == _brute_schedule(R, G, capacity, 1000)
    flushes, tails, grows, captures = got
    assert flushes == list(range(R, 1001, R)) and tails == [R * (k + 1) for k in range(len(flushes))]
    assert grows == max(0, math.ceil(math.log2(max(tails[-1], capacity) / capacity))) and captures in (grows, grows + 1)
    assert quant_flush(R - 1, 0, capacity, R) == (0, 0) and quant_flush(R, capacity, capacity, R) == (R, 1)
    assert quant_flush(R, capacity - R, capacity, R) == (R, 0)


def test_issue_end_to_end_setup_has_four_flushes_and_two_grows():
    from kvcache_factory_amd.cache import quant_schedule
    assert quant_schedule(64, 64, 300) == ([64, 128, 192, 256], [64, 128, 192, 256], 2, 3)
    assert quant_schedule(64, 64, 80) == ([64], [64], 0, 1)


# ---- 3. the adapter: decode_step_quant's signature over a device-counted entry ------------------------------------------------------------
def adapter(step_dev, capacity_of, seen=None):
    """fn with decode_step_quant's signature: the case's quantized tail (Tq rows) and residual (T rows) go into buffers of
    capacity_of(Tq, T, t) = (tail capacity, residual capacity) rows — behind the rows in use code bytes are 0xFF, metadata NaN and
    residual rows NaN —, the two lengths into device words.  After the call the residual rows [0, T + t) are copied back into the
    case's buffers (which the harness then compares byte for byte), the words, the whole tail segment and everything behind the
    visible residual rows must be unchanged."""
    def run(q, kn, vn, prefix, qtail, kr, vr, T, scaling, nbits, G, Rl):
        dev = q.device
        b, hkv, _, D = kr.shape
        t = q.shape[2]
        Tq = qtail[4] if qtail is not None else 0
        qcap, rcap = capacity_of(Tq, T, t)
        seg = None
        if qcap:
            kc = torch.full((b, hkv, qcap, D * nbits // 8), 0xFF, dtype=torch.uint8, device=dev)
            km = torch.full((b, hkv, -(-qcap // G), 2, D), float("nan"), dtype=torch.float32, device=dev)
            vm = torch.full((b, hkv, qcap, D // G, 2), float("nan"), dtype=torch.float32, device=dev)
            seg = [kc, kc.clone(), km, vm]
            if Tq:
                for new, old, rows in zip(seg, qtail[:4], (Tq, Tq, Tq // G, Tq)):
                    new[:, :, :rows] = old[:, :, :rows]
            before = [x.clone() for x in seg]
            seg = (*seg, 0)                                                  # the row count of the tuple is ignored
        bk = torch.full((b, hkv, rcap, D), float("nan"), dtype=kr.dtype, device=dev)
        bv = torch.full_like(bk, float("nan"))
        bk[:, :, :T], bv[:, :, :T] = kr[:, :, :T], vr[:, :, :T]
        words = torch.tensor([Tq, T], dtype=torch.int32, device=dev)
        out = step_dev(q, kn, vn, prefix, seg, bk, bv, words[0:1], words[1:2], scaling, nbits, G, Rl)
        kr[:, :, :T + t], vr[:, :, :T + t] = bk[:, :, :T + t], bv[:, :, :T + t]
        assert torch.isnan(bk[:, :, T + t:].float()).all() and torch.isnan(bv[:, :, T + t:].float()).all()
        assert words.tolist() == [Tq, T]                                     # the library only reads them
        if qcap:
            for x, y in zip(seg[:4], before):
                R._same_bytes(x, y, "the quantized tail")
        if seen is not None:
            seen.append(quant_dev_split_plan(b, q.shape[1], t, prefix[4], qcap, rcap)[0])
        return out
    return run


CAPS = {"own": lambda Tq, T, t: (Tq, T + t), "wide": lambda Tq, T, t: (Tq + 1024, T + t)}


def standin_decode_step_quant_dev(q, k_new, v_new, prefix, qtail, k_res, v_res, tail_word, res_word, scaling, nbits, group_size,
                                  residual_length, ws=None, out=None):
    """_kvc.decode_step_quant_dev restated: both words are clamped, then quant_ref's host-counted step at those lengths."""
    t = q.shape[2]
    qcap = qtail[0].shape[2] if qtail is not None else 0
    Tq = min(max(int(tail_word.reshape(-1)[0]), 0), qcap)
    Rr = min(max(int(res_word.reshape(-1)[0]), 0), k_res.shape[2] - t)
    seg = (*qtail[:4], Tq) if Tq else None
    o = Q.decode_step_quant(q, k_new, v_new, prefix, seg, k_res, v_res, Rr, scaling, nbits, group_size, residual_length)
    if out is not None:
        out.copy_(o)
        return out
    return o


QSPECS = [s for s in R.GRID if s["entry"] == "quant"]
SMALL = [s for s in QSPECS if s["P"] + s["Tq"] + s["T"] + s["t"] <= 200]     # the short cases: every code width, every dtype


def test_there_are_small_cases_of_every_width_and_dtype():
    assert {s["nbits"] for s in SMALL} == {2, 4, 8} and {s["dtype"] for s in SMALL} == {R.BF16, R.FP16, R.FP32}


@pytest.mark.parametrize("cap", list(CAPS))
@pytest.mark.parametrize("spec", SMALL, ids=[R.spec_id(s) for s in SMALL])
def test_adapter_over_the_standin_passes_both_families(spec, cap):
    seen = []
    fn = adapter(standin_decode_step_quant_dev, CAPS[cap], seen)
    assert run_needles(spec, fn) > 0
    assert cap == "own" or min(seen) > 1                                     # the wide bound is a split plan
    e_kernel, e_ref = run_bound(spec, fn)
    assert e_kernel <= R.FACTOR * e_ref


def test_adapter_notices_a_write_behind_the_visible_rows_and_a_touched_word():
    spec = SMALL[0]

    def scribbles(q, kn, vn, prefix, qtail, kr, vr, tw, rw, *a, **kw):
        out = standin_decode_step_quant_dev(q, kn, vn, prefix, qtail, kr, vr, tw, rw, *a, **kw)
        kr[:, :, -1] = 0
        return out

    def counts(q, kn, vn, prefix, qtail, kr, vr, tw, rw, *a, **kw):
        out = standin_decode_step_quant_dev(q, kn, vn, prefix, qtail, kr, vr, tw, rw, *a, **kw)
        rw.add_(1)
        return out

    def dirties_tail(q, kn, vn, prefix, qtail, kr, vr, tw, rw, *a, **kw):
        qtail[0][:, :, -1] = 0
        return standin_decode_step_quant_dev(q, kn, vn, prefix, qtail, kr, vr, tw, rw, *a, **kw)
    for bad, cap in ((scribbles, lambda Tq, T, t: (Tq, T + t + 2)), (counts, CAPS["own"]), (dirties_tail, CAPS["wide"])):
        with pytest.raises(AssertionError):
            run_bound(spec, adapter(bad, cap))


# ---- 4. the layer and the decoder on stand-ins ----------------------------------------------------------------------------------------
@pytest.fixture()
def quant_kernels(cpu_kernels, monkeypatch):
    from kvcache_factory_amd import attention, graph_decode
    calls = []

    def spy(*a, **kw):
        calls.append((int(a[7][0]), int(a[8][0]), a[4][0].shape[2], kw.get("ws"), kw.get("out")))
        return standin_decode_step_quant_dev(*a, **kw)
    monkeypatch.setattr(_kvc, "decode_step_quant_dev", spy)
    monkeypatch.setattr(_kvc, "decode_quant_dev_plan", lambda *a, **kw: (None, 64))
    monkeypatch.setattr(_kvc, "quantize_rows", Q.quantize_rows)
    monkeypatch.setattr(_kvc, "dequantize_rows", Q.dequantize_rows)
    monkeypatch.setattr(_kvc, "decode_step_quant", Q.decode_step_quant)
    real = attention._fusable
    monkeypatch.setattr(graph_decode, "_on_gpu", lambda t: True)
    monkeypatch.setattr(attention, "_fusable", lambda module, layer, h, m, kw: True if not h.is_cuda else real(module, layer, h, m, kw))
    yield calls


def test_decoder_flush_points_mirrors_and_the_host_issued_bytes(quant_kernels):
    """nbits 4, G 32, R 32, first capacity 32, 75 tokens: flushes after steps 32 and 64, one grow; the mirrors and the words after every
    step; and the layer's bytes equal those of QuantizedCompressedCache teacher-forced with the same tokens (the same stand-ins)."""
    from kvcache_factory_amd import GraphDecoder, QuantizedCompressedCache
    from kvcache_factory_amd.cache import QuantizedDeviceLayer, quant_schedule
    ids, steps = _prompts((40,), seed=3)[0], 75
    with _Patched("snapkv") as model:
        dec = GraphDecoder(model, nbits=4, q_group_size=32, residual_length=32, tail_rows=20, capture=False)
        assert dec.tail_rows == 32                                           # rounded up to a whole residual
        logits = [dec.prefill(ids).clone()]
        assert all(type(layer) is QuantizedDeviceLayer for layer in dec._cache.layers) and dec._counter.tolist() == [[0, 0], [0, 0]]
        toks, grew_at = [], []
        for j in range(steps):
            toks.append(logits[-1][:, -1].argmax(-1, keepdim=True))
            g0 = dec.grows
            logits.append(dec.step(toks[-1]).clone())
            if dec.grows != g0:
                grew_at.append(j + 1)
            n = j + 1
            for i, layer in enumerate(dec._cache.layers):
                assert layer.rows() == (16, n // 32 * 32, n % 32) and layer.get_seq_length() == 41 + j == dec._cache.get_seq_length()
                assert layer.stored_length() == 16 + n and layer.keys.shape == (1, 4, 16 + n, 64) and layer.get_mask_sizes(1) == (17 + n, 0)
                assert dec._counter[:, i].tolist() == [n // 32 * 32, n % 32]
        flushes, tails, grows, _ = quant_schedule(32, 32, steps)
        assert (flushes, tails, grows) == ([32, 64], [32, 64], 1) and grew_at == [64] and dec.grows == 1 and dec._capacity == 64
        assert [c[:3] for c in quant_kernels[:6:2]] == [(0, 0, 32), (0, 1, 32), (0, 2, 32)] and quant_kernels[-1][:3] == (64, 10, 64)
        assert all(c[3] is not None and c[4] is not None for c in quant_kernels)           # its own workspace and output, never the pool
        assert len({c[4].data_ptr() for c in quant_kernels}) == 2                           # one output buffer per layer
        cache = QuantizedCompressedCache(model.config, nbits=4, q_group_size=32, residual_length=32)
        with torch.no_grad():
            model(ids, past_key_values=cache, use_cache=True)
            for tok in toks:
                model(tok, past_key_values=cache, use_cache=True)
        for mine, ref in zip(dec._cache.layers, cache.layers):
            (pre, qt, (rk, rv, rr)) = mine.segments()
            assert (pre[4], qt[4], rr) == (ref._prows, ref._trows, ref._rrows) == (16, 64, 11)
            for x, y, rows in zip(pre[:4] + qt[:4], (ref._pkc, ref._pvc, ref._pkm, ref._pvm, ref._tkc, ref._tvc, ref._tkm, ref._tvm),
                                  (16, 16, 1, 16, 64, 64, 2, 64)):
                R._same_bytes(x[:, :, :rows], y[:, :, :rows], "codes / metadata")
            R._same_bytes(rk[:, :, :rr], ref._rk[:, :, :rr], "residual keys")
            R._same_bytes(rv[:, :, :rr], ref._rv[:, :, :rr], "residual values")
            R._same_bytes(mine.keys, ref.keys, "keys view")
        layer = dec._cache.layers[0]
        for op in (lambda: layer.update(ids, ids), lambda: layer.crop(3), lambda: layer.reorder_cache(torch.zeros(1, dtype=torch.long)),
                   lambda: layer.batch_repeat_interleave(2), lambda: layer.prefill(None, None, 0), lambda: layer.grow_tail(),
                   lambda: layer.enter_device_length(None, 4, 2)):
            with pytest.raises(NotImplementedError):
                op()


def test_decoder_refusals_raise_before_anything_is_stored(quant_kernels):
    from kvcache_factory_amd import GraphDecoder, KVQuantCompressedCache, QuantizedCompressedCache
    from transformers import DynamicCache
    ids = _prompts((40,))[0]
    with _Patched("snapkv") as model:
        for kw, msg in ((dict(nbits=3), "nbits"), (dict(nbits=4, q_group_size=48), "q_group_size"),
                        (dict(nbits=4, q_group_size=64, residual_length=96), "residual_length"),
                        (dict(nbits=4, interval=8), "not both"), (dict(nbits=4, heavy_hitter=8), "not both")):
            with pytest.raises(ValueError, match=msg):
                GraphDecoder(model, **kw)
        dec = GraphDecoder(model, nbits=4, q_group_size=32, residual_length=32, capture=False)
        cache = DynamicCache(config=model.config)
        with pytest.raises(ValueError, match="past_key_values"):
            dec.prefill(ids, past_key_values=cache)
        with pytest.raises(NotImplementedError, match="one sequence"):
            dec.prefill(torch.cat([ids, ids]))
        for cache in (QuantizedCompressedCache(model.config, nbits=4), KVQuantCompressedCache(model.config, nbits=4)):
            with pytest.raises(NotImplementedError, match="quantized"):     # refused exactly as without nbits
                dec.prefill(ids, past_key_values=cache)
            assert all(layer.get_seq_length() == 0 for layer in cache.layers)
        assert dec._cache is None and dec._graph is None and dec.captures == 0 and cache.get_seq_length() == 0
    for method in ("adakv", "headkv", "think"):
        with _Patched(method) as model:
            with pytest.raises(NotImplementedError, match=method):
                GraphDecoder(model, nbits=4)
    with _Patched("snapkv", merge="pivot") as model:
        with pytest.raises(NotImplementedError, match="merge"):
            GraphDecoder(model, nbits=4)
    for method in ("pyramidkv", "streamingllm", "h2o", "l2norm", "cam"):   # the methods the quantized cache takes are constructed
        with _Patched(method) as model:
            assert GraphDecoder(model, nbits=2, capture=False).nbits == 2


def test_nbits_none_changes_nothing(quant_kernels):
    from kvcache_factory_amd import GraphDecoder
    with _Patched("snapkv") as model:
        dec = GraphDecoder(model, tail_rows=5)
        assert dec.nbits is None and dec.tail_rows == 5
