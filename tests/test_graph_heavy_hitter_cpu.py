"""Heavy-hitter eviction under graph-replayed decoding, without a GPU: kvc_decode_step_dev_scored is declared, exported and checks its
arguments before any launch; its workspace against the restated plan of the bound; a restatement of the entry (heavy_hitter_ref's
rule 2 plus the device-length rules) through the decode-step conformance harness; BoundedHeavyHitterLayer driven beside
HeavyHitterLayer on the same rows with the kernels replaced by stand-ins; GraphDecoder(model, heavy_hitter=N) with capture=False on a
tiny patched Llama — the mirrors, the per-layer counters, the prefix-length words, the refusals."""
import ctypes
import os
import re

import pytest
import torch

import decode_ref as DR
import heavy_hitter_ref as R
from kvcache_factory_amd import _kvc
from test_batch_generation_cpu import _prompts
from test_decode_conformance_cpu import run_bound, run_needles
from test_graph_compress_cpu import CAP, N_LAYERS, WIN, _Patched, _config
from test_graph_decode_cpu import dev_split_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kvc_decode_dev_scored_workspace_bytes", "kvc_decode_step_dev_scored")
SCORED = [s for s in DR.GRID if s["entry"] == "scored"]
CAPS = {"own": lambda T, t: T + t, "wide": lambda T, t: T + t + 1024}       # the case's own rows; a bound that forces several splits


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- the entry, restated ---------------------------------------------------------------------------------------------------------------
def restated_decode_step_dev_scored(q, k_new, v_new, k_prefix, v_prefix, prefix_rows, k_tail, v_tail, tail_counter, score_prefix,
                                    score_tail, scaling, rows_b=None, ws=None, out=None):
    """_kvc.decode_step_dev_scored restated: T is the counter clamped to [0, capacity - t], P_b the per-row word clamped to
    [0, prefix_rows]; then heavy_hitter_ref's rule 2 over virtual_rows at those lengths, in fp32 (the arithmetic of
    heavy_hitter_ref.standin_decode_step_scored, operation for operation)."""
    b, hq, t, D = q.shape
    G = hq // k_new.shape[1]
    T = min(max(int(tail_counter.reshape(-1)[0]), 0), k_tail.shape[2] - t)
    k_tail[:, :, T:T + t] = k_new
    v_tail[:, :, T:T + t] = v_new
    score_tail[:, :, T:T + t] = 0
    res = torch.empty(b, t, hq, D, dtype=q.dtype)
    for bi in range(b):
        s = slice(bi, bi + 1)
        P = prefix_rows if rows_b is None else min(max(int(rows_b[bi]), 0), prefix_rows)
        probs = R.step_probs(q[s], k_prefix[s], k_tail[s], P, T, scaling, torch.float32)
        V = R.virtual_rows(v_prefix[s], v_tail[s], P, T + t, G).float()
        outs = []
        for i, p in enumerate(probs):
            score_prefix[s, :, :P] += p[:, :, :P]
            score_tail[s, :, :T + i + 1] += p[:, :, P:]
            outs.append(torch.einsum("bhr,bhrd->bhd", p, V[:, :, :P + T + i + 1])[:, :, None])
        res[s] = torch.cat(outs, 2).transpose(1, 2).to(q.dtype)
    if out is not None:
        out.copy_(res)
        return out
    return res


def scored_adapter(fn, capacity_of, seen=None):
    """decode_step_scored's signature over decode_step_dev_scored (`fn`): the case's tail rows [0, T) go into NaN-filled K / V buffers
    of capacity_of(T, t) rows, their scores into a NaN-filled score tail of as many slots, T into a counter and the prefix length into
    a per-row word.  After the call rows [0, T + t) are copied back into the case's buffers (which the harness compares: appended rows
    byte for byte, the scores by check_scores) and everything behind them must still be NaN, the counter and the word unchanged."""
    def run(q, kn, vn, kp, vp, P, kt, vt, T, sp, st, scaling):
        b, hkv, _, D = kt.shape
        hq, t, dev = q.shape[1], q.shape[2], kt.device
        cap = capacity_of(T, t)
        bk = torch.full((b, hkv, cap, D), float("nan"), dtype=kt.dtype, device=dev)
        bv = torch.full_like(bk, float("nan"))
        bs = torch.full((b, hq, cap), float("nan"), dtype=torch.float32, device=dev)
        bk[:, :, :T], bv[:, :, :T], bs[:, :, :T] = kt[:, :, :T], vt[:, :, :T], st[:, :, :T]
        counter = torch.tensor([T], dtype=torch.int32, device=dev)
        rows_b = torch.full((b,), P, dtype=torch.int32, device=dev)
        out = fn(q, kn, vn, kp, vp, P, bk, bv, counter, sp, bs, scaling, rows_b=rows_b)
        kt[:, :, :T + t], vt[:, :, :T + t], st[:, :, :T + t] = bk[:, :, :T + t], bv[:, :, :T + t], bs[:, :, :T + t]
        assert torch.isnan(bk[:, :, T + t:].float()).all() and torch.isnan(bv[:, :, T + t:].float()).all()
        assert torch.isnan(bs[:, :, T + t:]).all()
        assert int(counter) == T and rows_b.tolist() == [P] * b              # the library only reads them
        if seen is not None:
            seen.append(dev_split_plan(b, hq, t, P, cap)[0])
        return out
    return run


# ---- 1. header, binding ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_exports_the_entry(kvc):
    header = open(os.path.join(ROOT, "include", "kvc.h")).read()
    L = kvc.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header) and name in kvc.EXPORTS
        getattr(L, name)
    assert L.kvc_version() == 5 == int(re.search(r"#define\s+KVC_VERSION\s+(\d+)", header).group(1))
    doc = header[header.index("/* kvc_decode_step_dev_scored:"):header.index("int kvc_decode_step_dev_scored(")]
    assert "clamp(*tail_rows_dev, 0, tail_capacity - new_rows)" in doc and "exp2(s - M) / Lsum" in doc
    assert callable(kvc.decode_step_dev_scored) and callable(kvc.decode_dev_scored_plan)


# ---- 2. argument checks: an error text and no launch ----------------------------------------------------------------------------------------
P_, CAP_ = 40, 216                                                          # test_graph_decode_cpu._dp's layout: hq 8, hkv 2, D 128


def _sp(kvc, **kw):
    sp = kvc.DecodeScoredParams()
    base = dict(dtype=kvc.BF16, bsz=1, n_q_heads=8, n_kv_heads=2, head_dim=128, prefix_rows=P_, tail_rows=0, new_rows=1, scaling=0.1,
                q_stride_b=1024, q_stride_h=128, q_stride_l=128, new_stride_b=256, new_stride_h=128, new_stride_l=128,
                prefix_stride_b=8 * 48 * 128, prefix_stride_h=48 * 128, tail_stride_b=2 * CAP_ * 128, tail_stride_h=CAP_ * 128,
                out_stride_b=1024, out_stride_h=128, out_stride_l=1024)
    score = dict(score_prefix_stride_b=8 * 48, score_prefix_stride_h=48, score_tail_stride_b=8 * CAP_, score_tail_stride_h=CAP_)
    for k, v in {**base, **score, **kw}.items():
        setattr(sp if k in score else sp.step, k, v)
    return sp


NAMES = ("counter", "rows_b", "q", "k_new", "v_new", "k_prefix", "v_prefix", "k_tail", "v_tail", "score_prefix", "score_tail", "out", "ws")
BASE = 1 << 40


def _call(L, sp, cap=CAP_, ws_bytes=0, **ptr):
    """The entry with never-dereferenced pointers 16 MiB apart (so nothing overlaps unless a case says so).  No call here is valid
    to the end: one that passes every other check stops at the workspace, which is too small by default."""
    addr = {n: BASE + (i << 24) for i, n in enumerate(NAMES)}
    addr["rows_b"] = None
    addr.update(ptr)
    args = [None if addr[n] is None else ctypes.c_void_p(addr[n]) for n in NAMES]
    return L.kvc_decode_step_dev_scored(ctypes.byref(sp) if sp is not None else None, cap, *args, ws_bytes, None)


@pytest.mark.parametrize("kw,cap,code,msg", [
    (dict(new_rows=3), 2, -1, b"tail_capacity"), (dict(), 0, -1, b"tail_capacity"), (dict(), -7, -1, b"tail_capacity"),
    (dict(head_dim=96), CAP_, -2, b"head_dim"), (dict(dtype=7), CAP_, -1, b"dtype"), (dict(n_q_heads=7), CAP_, -1, b"head counts"),
    (dict(new_rows=0), CAP_, -1, b"row counts"), (dict(prefix_rows=-1), CAP_, -1, b"row counts"),
    (dict(prefix_rows=2 ** 31 - 100, score_prefix_stride_h=2 ** 31, score_prefix_stride_b=2 ** 34), CAP_, -1, b"overflows"),
    (dict(score_prefix_stride_h=P_ - 1), CAP_, -1, b"score_prefix strides"), (dict(score_prefix_stride_b=7 * 48), CAP_, -1, b"score_prefix strides"),
    (dict(score_tail_stride_h=CAP_ - 1), CAP_, -1, b"score_tail strides"), (dict(score_tail_stride_b=7 * CAP_), CAP_, -1, b"score_tail strides"),
])
def test_entry_rejects_invalid_params_before_any_pointer(kvc, kw, cap, code, msg):
    L = kvc.lib()
    sp = _sp(kvc, **kw)
    assert _call(L, sp, cap) == code and msg in L.kvc_last_error(), L.kvc_last_error()
    assert L.kvc_decode_dev_scored_workspace_bytes(ctypes.byref(sp), cap) == 0 and msg in L.kvc_last_error()


def test_entry_rejects_null_misaligned_and_aliased_pointers(kvc):
    L = kvc.lib()
    sp = _sp(kvc)
    need = L.kvc_decode_dev_scored_workspace_bytes(ctypes.byref(sp), CAP_)
    assert need > 0 and need % 16 == 0 and L.kvc_last_error() == b""
    assert _call(L, None) == -1 and b"NULL" in L.kvc_last_error() and L.kvc_decode_dev_scored_workspace_bytes(None, CAP_) == 0
    # kvc_decode_step_dev's checks, kept
    assert _call(L, sp, counter=None) == -1 and b"tail_rows_dev" in L.kvc_last_error()
    assert _call(L, sp, counter=BASE + 2) == -4 and b"tail_rows_dev" in L.kvc_last_error()
    assert _call(L, sp, rows_b=BASE + (1 << 24) + 2) == -4 and b"prefix_rows_b" in L.kvc_last_error()
    for name in ("q", "k_new", "v_new", "k_prefix", "v_prefix", "k_tail", "v_tail", "out"):
        assert _call(L, sp, **{name: None}) == -1 and b"non-NULL" in L.kvc_last_error(), name
        assert _call(L, sp, **{name: BASE + (NAMES.index(name) << 24) + 8}) == -4 and b"16-byte" in L.kvc_last_error(), name
    assert _call(L, _sp(kvc, tail_stride_h=CAP_ * 128 + 4)) == -4 and b"stride" in L.kvc_last_error()
    # the scores
    for name in ("score_prefix", "score_tail"):
        assert _call(L, sp, **{name: None}) == -1 and b"score" in L.kvc_last_error() and b"non-NULL" in L.kvc_last_error(), name
        assert _call(L, sp, **{name: BASE + (NAMES.index(name) << 24) + 2}) == -4 and b"4-byte" in L.kvc_last_error(), name
    at = lambda n: BASE + (NAMES.index(n) << 24)                             # noqa: E731
    last_tail = ((8 - 1) * CAP_ + CAP_ - 1) * 4                             # byte offset of score_tail's last slot
    for kw in (dict(score_tail=at("score_prefix")), dict(score_prefix=at("score_tail") + last_tail), dict(out=at("score_tail") + last_tail - 12),
               dict(score_prefix=at("out") + 8 * 128 * 2 - 4), dict(score_tail=at("out") + 256)):
        assert _call(L, sp, **kw) == -1 and b"overlap" in L.kvc_last_error(), kw
    assert _call(L, sp, score_prefix=at("score_tail") + last_tail + 4) == -3 and b"too small" in L.kvc_last_error()   # one slot on: disjoint
    # the workspace is required in full: kvc_decode_step_scored's errors
    assert _call(L, sp, ws=None, ws_bytes=need) == -3 and b"NULL" in L.kvc_last_error()
    assert _call(L, sp, ws=at("ws") + 8, ws_bytes=need) == -3 and b"aligned" in L.kvc_last_error()
    assert _call(L, sp, ws_bytes=need - 16) == -3 and b"too small" in L.kvc_last_error()
    # an empty prefix needs neither prefix pointers nor score_prefix; p->tail_rows is ignored, whatever it holds
    p0 = _sp(kvc, prefix_rows=0)
    assert _call(L, p0, k_prefix=None, v_prefix=None, score_prefix=None, ws=None, ws_bytes=0) == -3
    for kw in (dict(tail_rows=-9), dict(tail_rows=10 ** 9)):
        assert L.kvc_decode_dev_scored_workspace_bytes(ctypes.byref(_sp(kvc, **kw)), CAP_) == need, kw


# ---- 3. the workspace follows the bound's plan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hq,t,D,P,cap", [(8, 1, 128, 40, 216), (8, 3, 64, 40, 216), (32, 1, 128, 136, 64), (32, 1, 128, 2056, 128),
                                          (32, 1, 128, 128, 128), (4, 1, 64, 0, 1), (4, 5, 64, 7, 5), (2, 1, 64, 9000, 4096), (8, 1, 64, 64, 24)])
def test_workspace_is_every_split_s_partials_plus_the_logits(kvc, hq, t, D, P, cap):
    L = kvc.lib()
    splits, rps = dev_split_plan(1, hq, t, P, cap)
    al = lambda n: -(-n // 16) * 16                                          # noqa: E731
    want = al(hq * t * splits * (D + 2) * 4) + al(hq * t * (P + cap) * 4)    # (M, Lsum, acc[D]) with one split too; logits by virtual row
    seen = set()
    for tail_rows in (0, 1, cap - t, cap + 1000, -3):                        # the host's idea of the tail changes nothing
        sp = _sp(kvc, n_q_heads=hq, n_kv_heads=hq // 2, head_dim=D, prefix_rows=P, new_rows=t, tail_rows=tail_rows,
                 score_prefix_stride_h=P, score_prefix_stride_b=hq * P, score_tail_stride_h=cap, score_tail_stride_b=hq * cap)
        seen.add(L.kvc_decode_dev_scored_workspace_bytes(ctypes.byref(sp), cap))
    assert seen == {want}
    q, kn = torch.zeros(1, hq, t, D, dtype=torch.bfloat16), torch.zeros(1, hq // 2, t, D, dtype=torch.bfloat16)
    kp, kt = torch.zeros(1, hq, max(P, 1), D, dtype=torch.bfloat16), torch.zeros(1, hq // 2, cap, D, dtype=torch.bfloat16)
    s_p, s_t = torch.zeros(1, hq, max(P, 1)), torch.zeros(1, hq, cap)
    assert kvc.decode_dev_scored_plan(q, kn, kp, P, kt, s_p if P else None, s_t)[1] == want


# ---- 4. the restatement through the conformance harness ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", list(CAPS))
@pytest.mark.parametrize("spec", SCORED, ids=[DR.spec_id(s) for s in SCORED])
def test_restatement_passes_both_families(spec, cap):
    fn = scored_adapter(restated_decode_step_dev_scored, CAPS[cap])
    rows = spec["P"] + spec["T"] + spec["t"]
    assert run_needles(spec, fn) >= (rows if rows <= 320 else rows // 16)    # check_scores included (entry "scored")
    e_kernel, e_ref = run_bound(spec, fn)
    assert e_kernel <= DR.FACTOR * e_ref


def test_restatement_follows_the_device_length_rules():
    """The clamp of the counter and of the prefix word, the tail mapped to r - P_b, slots behind the visible rows left alone."""
    g = torch.Generator().manual_seed(2)
    bf = lambda *sh: torch.randn(*sh, generator=g).to(torch.bfloat16)       # noqa: E731
    hq, hkv, D, pcap, cap = 4, 2, 64, 12, 6
    q, kn, vn, kp, vp = bf(1, hq, 1, D), bf(1, hkv, 1, D), bf(1, hkv, 1, D), bf(1, hq, pcap, D), bf(1, hq, pcap, D)
    for counter, plen, T, P in ((-5, 99, 0, 12), (cap + 100, -1, cap - 1, 0), (3, 7, 3, 7)):
        kt, vt = bf(1, hkv, cap, D), bf(1, hkv, cap, D)
        sp, st = torch.rand(1, hq, pcap, generator=g), torch.rand(1, hq, cap, generator=g)
        sp0, st0, kt0 = sp.clone(), st.clone(), kt.clone()
        out = restated_decode_step_dev_scored(q, kn, vn, kp, vp, pcap, kt, vt, torch.tensor([counter], dtype=torch.int32), sp, st, 0.125,
                                              rows_b=torch.tensor([plen], dtype=torch.int32))
        assert torch.equal(kt[:, :, T], kn[:, :, 0]) and torch.equal(kt[:, :, :T], kt0[:, :, :T]) and torch.equal(kt[:, :, T + 1:], kt0[:, :, T + 1:])
        assert torch.equal(sp[:, :, P:], sp0[:, :, P:]) and torch.equal(st[:, :, T + 1:], st0[:, :, T + 1:])
        inc = torch.cat([sp[:, :, :P] - sp0[:, :, :P], st[:, :, :T] - st0[:, :, :T], st[:, :, T:T + 1]], 2)
        assert torch.allclose(inc.sum(-1), torch.ones(1, hq), atol=1e-4) and bool((inc > -1e-6).all())
        ref = R.standin_decode_step_scored(q, kn, vn, kp, vp, P, kt0.clone(), vt.clone(), T, sp0.clone(), st0.clone(), 0.125)
        assert torch.equal(_bits(out), _bits(ref))


# ---- 5. the bounded layer beside the host-counted one ---------------------------------------------------------------------------------------
@pytest.fixture()
def hh_kernels(monkeypatch):
    monkeypatch.setattr(_kvc, "decode_step_scored", R.standin_decode_step_scored)
    monkeypatch.setattr(_kvc, "decode_step_dev_scored", restated_decode_step_dev_scored)
    monkeypatch.setattr(_kvc, "decode_evict", R.standin_decode_evict)
    monkeypatch.setattr(_kvc, "compress", R.standin_compress)
    R.EVICTIONS.clear()
    yield


def _bf(g, *sh):
    return torch.randn(*sh, generator=g).to(torch.bfloat16)


def _h2o(cap=40, W=8, **kw):
    from kvcache_factory_amd import pyramidkv_utils as pu
    return pu.H2OKVCluster(window_size=W, max_capacity_prompt=cap, **kw)


def _twins(g, P0, interval, cl, hq=4, hkv=2, D=64):
    """Two HeavyHitterLayers prefilled alike: P0 rows with random scores, or ("pass") a 20-token prompt through prefill_heavy_hitter's
    pass-through branch (K / V repeat_kv-expanded, every score 0)."""
    from kvcache_factory_amd import HeavyHitterLayer, pyramidkv_utils as pu
    a, b = HeavyHitterLayer(interval), HeavyHitterLayer(interval)
    if P0 == "pass":
        q, k, v = _bf(g, 1, hq, 20, D), _bf(g, 1, hkv, 20, D), _bf(g, 1, hkv, 20, D)
        for x in (a, b):
            pu.prefill_heavy_hitter(cl, x, k, q, v)
        assert a.rows() == (20, 0) and float(a.scores().abs().sum()) == 0
        return a, b
    k, v, s = _bf(g, 1, hq, P0, D), _bf(g, 1, hq, P0, D), torch.rand(1, hq, P0, generator=g) * 5
    for x in (a, b):
        x.prefill(k.clone(), v.clone(), 1000)
        x._sbuf[:, :, :P0] = s
    return a, b


def _addresses(layer):
    return [t.data_ptr() for t in (layer._kbuf, layer._vbuf, layer._sbuf, layer._ktail, layer._vtail, layer._stail, layer._plen,
                                   layer._kout, layer._vout, layer._sout, layer._dev_ws, layer._dev_counter)]


@pytest.mark.parametrize("P0", [20, 40, 45, "pass"])
def test_bounded_layer_follows_the_host_counted_layer(hh_kernels, P0):
    from kvcache_factory_amd.cache import BoundedHeavyHitterLayer, bounded_tail_rows, heavy_hitter_budget
    hq, hkv, D, interval = 4, 2, 64, 16
    cl = _h2o()
    B, W = heavy_hitter_budget(cl, interval)
    assert (B, W) == (40, 8)
    g = torch.Generator().manual_seed(3 + (P0 if P0 != "pass" else 0))
    host, seed = _twins(g, P0, interval, cl)
    p0, length0 = host.rows()[0], host.get_seq_length()
    counters = torch.full((3,), 77, dtype=torch.int32)
    layer = BoundedHeavyHitterLayer.adopt(seed, cl, interval, counters[1:2], hkv)
    cap = bounded_tail_rows(p0, B, interval)
    assert layer._kbuf.shape == (1, hq, max(p0, B), D) and layer._sbuf.shape == (1, hq, max(p0, B)) and layer._sbuf.dtype == torch.float32
    assert layer._ktail.shape == (1, hkv, cap, D) and layer._stail.shape == (1, hq, cap) and layer._stail.dtype == torch.float32
    assert layer._kout.shape == (1, hq, B, D) and layer._sout.shape == (1, hq, B) and layer._dev_ws.dtype == torch.uint8
    assert layer._dev_ws.numel() == _kvc.decode_dev_scored_plan(_bf(g, 1, hq, 1, D), _bf(g, 1, hkv, 1, D), layer._kbuf, max(p0, B),
                                                                 layer._ktail, layer._sbuf, layer._stail)[1] > 0
    assert counters.tolist() == [77, 0, 77] and int(layer._plen) == p0 and layer.get_seq_length() == length0 and layer.evictions == 0
    assert torch.equal(_bits(layer.scores()), _bits(host.scores())) and torch.equal(_bits(layer.keys), _bits(host.keys))
    addresses = _addresses(layer)
    at = []
    for step in range(56):                                                # P0 = 20: evictions after steps 36 and 52
        q, k, v = _bf(g, 1, hq, 1, D) * 1.5, _bf(g, 1, hkv, 1, D), _bf(g, 1, hkv, 1, D)
        n0 = host.evictions
        ref = host.decode_attend(q, k, v, D ** -0.5)
        out = layer.decode_attend(q, k, v, D ** -0.5)
        assert torch.equal(_bits(out), _bits(ref)), step
        assert layer._tail == int(counters[1])                               # the mirror is held: the owner advances it
        layer.after_decode(cl, q)                                            # nothing: the owner calls the trigger
        counters[1:2].add_(1)
        layer.advance(1)
        for x, y in ((layer.keys, host.keys), (layer.values, host.values), (layer.scores(), host.scores())):   # before the eviction
            assert torch.equal(_bits(x), _bits(y)), step
        host.after_decode(cl, q)
        did = layer.maybe_evict()
        assert did == (host.evictions > n0) and layer.evictions == host.evictions, step
        assert layer.stored_length() == host.stored_length() and layer.rows() == host.rows(), step
        assert layer.get_seq_length() == host.get_seq_length() == length0 + 1 + step
        assert int(layer._plen) == layer._stored and int(counters[1]) == layer._tail and counters[0] == counters[2] == 77
        for x, y in ((layer.keys, host.keys), (layer.values, host.values), (layer.scores(), host.scores())):
            assert torch.equal(_bits(x), _bits(y)), step
        if did:
            at.append(step)
            assert layer.rows() == (B, 0)
    assert len(at) >= 2 and at[0] == max(W, B + interval - p0) - 1 and at[1] - at[0] == interval and len(R.EVICTIONS) == 2 * len(at)
    assert addresses == _addresses(layer)                                    # every address, over at least two evictions


def test_bounded_layer_limits(hh_kernels):
    from kvcache_factory_amd import BoundedHeavyHitterLayer, HeavyHitterLayer
    from kvcache_factory_amd.cache import CompressedDynamicLayer
    g = torch.Generator().manual_seed(1)
    counter = torch.zeros(1, dtype=torch.int32)
    cl = _h2o()
    fresh = lambda interval=16: _twins(g, 40, interval, cl)[0]                # noqa: E731
    plain = CompressedDynamicLayer()
    plain.prefill(_bf(g, 1, 4, 40, 64), _bf(g, 1, 4, 40, 64), 100)
    with pytest.raises(NotImplementedError, match="CompressedDynamicLayer"):
        BoundedHeavyHitterLayer.adopt(plain, cl, 16, counter, 2)
    with pytest.raises(NotImplementedError, match="HeavyHitterLayer"):
        BoundedHeavyHitterLayer.adopt(HeavyHitterLayer(16), cl, 16, counter, 2)      # never prefilled
    used = fresh()
    used.decode_attend(_bf(g, 1, 4, 1, 64), _bf(g, 1, 2, 1, 64), _bf(g, 1, 2, 1, 64), 0.125)
    with pytest.raises(NotImplementedError, match="decoded rows"):
        BoundedHeavyHitterLayer.adopt(used, cl, 16, counter, 2)
    with pytest.raises(ValueError, match="HeavyHitterCache: interval 4 must be >= window_size 8"):
        BoundedHeavyHitterLayer.adopt(fresh(4), cl, 4, counter, 2)
    from kvcache_factory_amd import pyramidkv_utils as pu
    with pytest.raises(NotImplementedError, match="SnapKVCluster"):
        BoundedHeavyHitterLayer.adopt(fresh(), pu.SnapKVCluster(window_size=8, max_capacity_prompt=40), 16, counter, 2)
    with pytest.raises(NotImplementedError, match="merge='pivot'"):
        BoundedHeavyHitterLayer.adopt(fresh(), _h2o(merge="pivot"), 16, counter, 2)
    for bad in (0, -3, 1.5, True, None):
        with pytest.raises(ValueError, match="interval"):
            BoundedHeavyHitterLayer(bad)
    layer = BoundedHeavyHitterLayer.adopt(fresh(), cl, 16, counter, 2)
    with pytest.raises(NotImplementedError, match="fixed buffers"):
        layer.update(_bf(g, 1, 4, 1, 64), _bf(g, 1, 4, 1, 64))
    with pytest.raises(NotImplementedError, match="fixed buffers"):
        layer.reorder_cache(torch.tensor([0]))
    with pytest.raises(NotImplementedError, match="one-token"):
        layer.decode_attend(_bf(g, 1, 4, 2, 64), _bf(g, 1, 2, 2, 64), _bf(g, 1, 2, 2, 64), 0.125)
    with pytest.raises(NotImplementedError, match="never grows"):
        layer.grow_tail()
    with pytest.raises(NotImplementedError, match="BoundedHeavyHitterLayer"):
        layer.enter_device_length(counter, 4, 2)
    with pytest.raises(NotImplementedError, match="adopt"):
        layer.prefill(_bf(g, 1, 4, 40, 64), _bf(g, 1, 4, 40, 64), 40)
    for _ in range(layer.tail_capacity()):                                   # an owner that never calls maybe_evict: the tail fills up
        layer.decode_attend(_bf(g, 1, 4, 1, 64), _bf(g, 1, 2, 1, 64), _bf(g, 1, 2, 1, 64), 0.125)
        layer.advance(1)
    with pytest.raises(RuntimeError, match="maybe_evict"):
        layer.decode_attend(_bf(g, 1, 4, 1, 64), _bf(g, 1, 2, 1, 64), _bf(g, 1, 2, 1, 64), 0.125)


def test_the_budget_rule_is_stated_once():
    from kvcache_factory_amd import HeavyHitterLayer
    from kvcache_factory_amd.cache import heavy_hitter_budget
    cl = _h2o(cap=24, W=8)
    assert HeavyHitterLayer(16).budget(cl) == heavy_hitter_budget(cl, 16) == (24, 8)
    for interval in (4, 7):
        for fn in (lambda: HeavyHitterLayer(interval).budget(cl), lambda: heavy_hitter_budget(cl, interval)):
            with pytest.raises(ValueError, match=f"HeavyHitterCache: interval {interval} must be >= window_size 8"):
                fn()


# ---- 6. GraphDecoder(model, heavy_hitter=N), capture=False -------------------------------------------------------------------------------
@pytest.fixture()
def cpu_decoder(hh_kernels, monkeypatch):
    """The GPU-only gates opened for the stand-in kernels: the patched forward takes the fused step on CPU tensors."""
    from kvcache_factory_amd import attention, graph_decode
    real = attention._fusable
    monkeypatch.setattr(graph_decode, "_on_gpu", lambda t: True)
    monkeypatch.setattr(attention, "_fusable", lambda module, layer, h, m, kw: True if not h.is_cuda else real(module, layer, h, m, kw))
    yield


@pytest.mark.parametrize("L", [40, 10])                                      # a compressed prompt; a pass-through one (L < CAP)
def test_decoder_follows_the_schedule(cpu_decoder, L):
    from kvcache_factory_amd import BoundedHeavyHitterLayer, GraphDecoder
    from kvcache_factory_amd.cache import bounded_tail_rows, decode_trigger
    N, steps = 8, 45
    ids = _prompts((L,), seed=3)[0]
    with _Patched("h2o") as model:
        dec = GraphDecoder(model, heavy_hitter=N, capture=False)
        assert dec.heavy_hitter == N and dec.interval is None
        logits = dec.prefill(ids)
        layers = dec._cache.layers
        assert len(layers) == N_LAYERS and all(type(x) is BoundedHeavyHitterLayer for x in layers) and tuple(layers) == dec._layers
        assert dec._counter.shape == (N_LAYERS,) and dec._counter.dtype == torch.int32 and dec._counter.tolist() == [0] * N_LAYERS
        P0 = min(L, CAP)
        assert all(x._plan == (CAP, WIN) and x.rows() == (P0, 0) and x.interval == N for x in layers)
        assert all(x.tail_capacity() == bounded_tail_rows(P0, CAP, N) for x in layers)
        for x in layers:                                                     # the prompt's column sums carried over (zeros: pass-through)
            s = x.scores()
            assert s.shape == (1, 4, P0) and (bool((s[:, :, :CAP - WIN] > 0).all()) if L >= CAP else float(s.abs().sum()) == 0)
        book, fired = [P0, 0], []
        for j in range(steps):
            tok = logits[:, -1].argmax(-1, keepdim=True)
            logits = dec.step(tok)
            book[1] += 1
            if decode_trigger(book[0], book[1], CAP, WIN, N):
                book = [CAP, 0]
                fired.append(j)
            for i, layer in enumerate(layers):
                assert [layer._stored, layer._tail] == book and int(layer._plen) == book[0], (j, i)
                assert layer._dev_counter.data_ptr() == dec._counter[i:i + 1].data_ptr() and layer.evictions == len(fired)
                assert layer.get_seq_length() == L + 1 + j and layer.stored_length() <= CAP + N
                assert layer.scores().shape == (1, 4, sum(book)) and bool((layer.scores() >= 0).all())
            assert dec._counter.tolist() == [book[1]] * N_LAYERS and dec._pos.tolist() == [[L + 1 + j]]
            assert dec._cache.get_seq_length() == L + 1 + j
        assert dec.grows == 0 and dec.captures == 0 and len(fired) >= 3
        assert len(R.EVICTIONS) == N_LAYERS * len(fired)
        out = GraphDecoder(model, heavy_hitter=N, capture=False).generate(ids, max_new_tokens=12)
        assert out.shape == (1, L + 12)


def test_decoder_refusals_raise_before_anything_is_stored(cpu_decoder):
    from transformers import DynamicCache
    from kvcache_factory_amd import GraphDecoder, HeavyHitterCache
    ids = _prompts((40,))[0]
    for method in ("snapkv", "pyramidkv", "streamingllm", "l2norm", "cam"):
        with _Patched(method) as model:
            with pytest.raises(NotImplementedError, match=method):
                GraphDecoder(model, heavy_hitter=8, capture=False)
            GraphDecoder(model, capture=False)                               # without the keyword: as before
    with _Patched("h2o", merge="pivot") as model:
        with pytest.raises(NotImplementedError, match="pivot"):
            GraphDecoder(model, heavy_hitter=8, capture=False)
    with _Patched("h2o") as model:
        for bad in (0, -1, True, 2.5, "8"):
            with pytest.raises(ValueError, match="heavy_hitter must be an int >= 1"):
                GraphDecoder(model, heavy_hitter=bad)
        with pytest.raises(ValueError, match="HeavyHitterCache: interval 3 must be >= window_size 4"):
            GraphDecoder(model, heavy_hitter=3)
        with pytest.raises(ValueError, match="not both"):
            GraphDecoder(model, heavy_hitter=8, interval=8)
        with pytest.raises(NotImplementedError, match="h2o"):               # interval= keeps refusing h2o
            GraphDecoder(model, interval=8)
        dec = GraphDecoder(model, heavy_hitter=8, capture=False)
        with pytest.raises(NotImplementedError, match="one sequence"):
            dec.prefill(torch.cat([ids, ids]))
        assert dec._cache is None and dec._counter is None
        for kw in (dict(), dict(heavy_hitter=8)):                            # a HeavyHitterCache handed over stays refused
            cache = HeavyHitterCache(_config(), interval=8)
            dec = GraphDecoder(model, capture=False, **kw)
            with pytest.raises(NotImplementedError, match="HeavyHitterCache"):
                dec.prefill(ids, past_key_values=cache)
            assert dec._cache is None and all(layer.get_seq_length() == 0 for layer in cache.layers)
        cache = DynamicCache(config=model.config)
        dec = GraphDecoder(model, heavy_hitter=8, capture=False)
        with pytest.raises(ValueError, match="past_key_values must be None"):
            dec.prefill(ids, past_key_values=cache)
        assert dec._cache is None and cache.get_seq_length() == 0
        for block in model.model.layers:                                     # the knobs can change after the decoder was built
            block.self_attn.config.merge = "pivot"
        with pytest.raises(NotImplementedError, match="pivot"):
            dec.prefill(ids)
        assert dec._cache is None
        for block in model.model.layers:
            block.self_attn.config.merge = None
            block.self_attn.config.window_size = 12
        with pytest.raises(ValueError, match="interval 8 must be >= window_size 12"):
            dec.prefill(ids)
        assert dec._cache is None
