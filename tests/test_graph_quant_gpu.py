"""The quantized cache under graph replay on the MI355X.

The entry (kvc_decode_step_quant_dev): the conformance harness of tests/decode_ref.py through the adapter of test_graph_quant_cpu.py
(the case's quantized tail and residual in larger buffers with 0xFF codes, NaN metadata and NaN rows behind the rows in use, both
lengths in device words: needles row-exact under the harness's rule for quantized rows, the per-element bound at the harness's
factor 4), the split edges of the bound-sized plan, bit identity with kvc_decode_step_quant where the two plans coincide, nothing
outside the visible rows matters, the clamps of both words between guard rows, and a captured call replayed across two split
boundaries and a flush against eager calls.
End to end (GraphDecoder(model, nbits=...) on the tiny Llama of the other GPU files): replay == eager byte for byte across flushes
and grow-and-re-capture events, flat memory and no host synchronisation during replays, PyramidKV, 2 and 8 bits, the bytes and the
logits of the host-issued QuantizedCompressedCache teacher-forced with the same tokens, the refusals."""
import collections

import pytest
import torch

import decode_ref as R
from test_decode_conformance_cpu import run_bound, run_needles
from test_graph_quant_cpu import CAPS, QSPECS, adapter, quant_dev_split_plan, visible_edges

pytestmark = pytest.mark.gpu

BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
RATIOS = collections.defaultdict(float)


def _bits(t):
    return t.contiguous().view(BITS[t.dtype])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- 1. conformance through the existing harness ------------------------------------------------------------------------------------------
CONF = [(s, c) for s in QSPECS for c in CAPS]
CONF_IDS = [f"{R.spec_id(s)}-{c}" for s, c in CONF]


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_needles_row_exact(kvc, gpu_device, spec, cap):
    seen = []
    probes = run_needles(spec, adapter(kvc.decode_step_quant_dev, CAPS[cap], seen), gpu_device)
    assert cap == "own" or min(seen) > 1                                     # the wide bound really ran split
    print(f"{R.spec_id(spec)} ({cap}, {max(seen)} splits): {probes} needles returned their row")


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_per_element_bound(kvc, gpu_device, spec, cap):
    e_kernel, e_ref = run_bound(spec, adapter(kvc.decode_step_quant_dev, CAPS[cap]), gpu_device)
    key = str(spec["dtype"])[6:]
    RATIOS[key] = max(RATIOS[key], e_kernel / e_ref)
    print(f"{R.spec_id(spec)} ({cap}): e_kernel / e_ref = {e_kernel / e_ref:.3f} (e_ref = {e_ref:.3e})")


def test_report_ratios():
    """The largest e_kernel / e_ref per dtype of this run (the bound allows 4; DESIGN.md section 4 records them)."""
    for dt, r in sorted(RATIOS.items()):
        print(f"e_kernel / e_ref  quant dev {dt:9s} {r:.3f}")
        assert r <= R.FACTOR


# ---- 2. split edges ---------------------------------------------------------------------------------------------------------------------------
HQ, HKV, P0, G, RL, QCAP, RCAP = 8, 2, 40, 32, 64, 128, 64
EDGE = [(dt, D, nb, t, Tq, Rr) for dt in (torch.bfloat16, torch.float32) for D in (128, 64) for nb in (2, 4) for t in (1, 3)
        for Tq, Rr in visible_edges(1, HQ, t, P0, QCAP, RCAP, G)]


def test_edge_set_is_the_plan_s():
    assert P0 + QCAP + RCAP == 232
    for t in (1, 3):
        assert quant_dev_split_plan(1, HQ, t, P0, QCAP, RCAP) == (4, 64)
        edges = set(visible_edges(1, HQ, t, P0, QCAP, RCAP, G))
        want = {(0, 0), (128, 64 - t)}
        for Tq, lo in ((0, 24), (64, 24), (32, 56), (128, 24)):
            want |= {(Tq, lo - (t - 1) - d) for d in (0, 1, 2)}                # the last token's visible rows: t - 1 more
        assert want <= edges, sorted(want - edges)
    assert {(0, 22), (0, 23), (0, 24), (64, 22), (64, 23), (64, 24), (32, 54), (32, 55), (32, 56), (128, 22), (128, 23), (128, 24),
            (128, 63)} <= set(visible_edges(1, HQ, 1, P0, QCAP, RCAP, G))


@pytest.mark.parametrize("dtype,D,nbits,t,Tq,Rr", EDGE, ids=[f"{str(e[0])[6:]}-D{e[1]}-{e[2]}b-t{e[3]}-Tq{e[4]}-R{e[5]}" for e in EDGE])
def test_split_edges(kvc, gpu_device, dtype, D, nbits, t, Tq, Rr):
    """fp64 attention under the harness bound and every row as a needle, at the lengths where the number of splits that run changes
    (tail capacity 128 and residual capacity 64 whatever Tq and Rr are: the plan is the bound's)."""
    spec = dict(entry="quant", dtype=dtype, D=D, hq=HQ, hkv=HKV, b=1, t=t, P=P0, Tq=Tq, T=Rr, nbits=nbits, G=G, R=RL)
    seen = []
    fn = adapter(kvc.decode_step_quant_dev, lambda Tq_, T_, t_: (QCAP, RCAP), seen)
    assert run_needles(spec, fn, gpu_device) >= P0 + Tq + Rr + t
    assert set(seen) == {4}
    e_kernel, e_ref = run_bound(spec, fn, gpu_device)
    print(f"Tq={Tq} Rr={Rr}: e_kernel / e_ref = {e_kernel / e_ref:.3f}")


# ---- direct calls -------------------------------------------------------------------------------------------------------------------------------
class _State:
    """q, k_new, v_new, a quantized prefix of `P` rows per query head, a quantized tail of `qcap` rows and a residual of `rcap` rows
    per KV head, all rows drawn and quantized by the library's own kvc_quantize_rows.  The tail segment and the residual are VIEWS
    into larger allocations with `guard` rows (key metadata: groups) of a sentinel on both sides of every head."""

    def __init__(self, kvc, dev, dtype, D, nbits, t, seed=0, guard=0, P=P0, qcap=QCAP, rcap=RCAP, hq=HQ, hkv=HKV):
        g = torch.Generator().manual_seed(seed)
        mk = lambda *sh: torch.randn(*sh, generator=g).to(dtype).to(dev)    # noqa: E731
        self.kvc, self.dtype, self.D, self.nbits, self.t, self.P, self.qcap, self.rcap, self.guard = kvc, dtype, D, nbits, t, P, qcap, rcap, guard
        self.q, self.kn, self.vn = mk(1, hq, t, D), mk(1, hkv, t, D), mk(1, hkv, t, D)
        self.pre = kvc.quant_buffers(1, hq, P, D, nbits, G, dev)
        kvc.quantize_rows(mk(1, hq, P, D), self.pre[0], self.pre[2], 0, kvc.QUANT_KEYS, nbits, G)
        kvc.quantize_rows(mk(1, hq, P, D), self.pre[1], self.pre[3], 0, kvc.QUANT_VALUES, nbits, G)
        gg = -(-guard // G)
        self.full = kvc.quant_buffers(1, hkv, guard + qcap + guard, D, nbits, G, dev)
        self.full = (*self.full[:2], torch.empty(1, hkv, gg + qcap // G + gg, 2, D, dtype=torch.float32, device=dev), self.full[3])
        self.rfull = [torch.empty(1, hkv, guard + rcap + guard, D, dtype=dtype, device=dev) for _ in range(2)]
        self.tail = (self.full[0][:, :, guard:guard + qcap], self.full[1][:, :, guard:guard + qcap],
                     self.full[2][:, :, gg:gg + qcap // G], self.full[3][:, :, guard:guard + qcap])
        self.rk, self.rv = (x[:, :, guard:guard + rcap] for x in self.rfull)
        self.live = kvc.quant_buffers(1, hkv, qcap, D, nbits, G, dev)          # the tail's rows, quantized group by group
        kvc.quantize_rows(mk(1, hkv, qcap, D), self.live[0], self.live[2], 0, kvc.QUANT_KEYS, nbits, G)
        kvc.quantize_rows(mk(1, hkv, qcap, D), self.live[1], self.live[3], 0, kvc.QUANT_VALUES, nbits, G)
        self.rlive = (mk(1, hkv, rcap, D), mk(1, hkv, rcap, D))
        self.words = torch.zeros(2, dtype=torch.int32, device=dev)
        self.ws = torch.empty(max(16, kvc.decode_quant_dev_plan(self.q, self.kn, (*self.pre, P), (*self.tail, 0), self.rk, nbits, G, RL)[1]),
                              dtype=torch.uint8, device=dev)

    def fill(self, Tq, Rr, code=0xFF, meta=float("nan"), row=float("nan")):
        """Rows [0, Tq) of the tail and [0, Rr) of the residual live, everything else (guards included) the given fillers."""
        for x, v in zip(self.full, (code, code, meta, meta)):
            x.fill_(v)
        for x in self.rfull:
            x.fill_(row)
        for x, y, rows in zip(self.tail, self.live, (Tq, Tq, -(-Tq // G), Tq)):
            x[:, :, :rows] = y[:, :, :rows]
        self.rk[:, :, :Rr], self.rv[:, :, :Rr] = self.rlive[0][:, :, :Rr], self.rlive[1][:, :, :Rr]
        return self

    def set(self, tw, rw):
        self.words.copy_(torch.tensor([tw, rw], dtype=torch.int32))
        return self

    def step(self, out=None, q=None, kn=None, vn=None):
        q, kn, vn = (self.q if q is None else q), (self.kn if kn is None else kn), (self.vn if vn is None else vn)
        return self.kvc.decode_step_quant_dev(q, kn, vn, (*self.pre, self.P), (*self.tail, 0), self.rk, self.rv, self.words[0:1],
                                              self.words[1:2], self.D ** -0.5, self.nbits, G, RL, ws=self.ws, out=out)

    def host_step(self, Tq, Rr):
        """kvc_decode_step_quant on the same state (its residual must hold a spare row beyond the step's: a copy)."""
        rk, rv = self.rk.contiguous().clone(), self.rv.contiguous().clone()
        qt = None if Tq == 0 else tuple(x.contiguous() for x in self.tail) + (Tq,)
        out = self.kvc.decode_step_quant(self.q, self.kn, self.vn, (*self.pre, self.P), qt, rk, rv, Rr, self.D ** -0.5, self.nbits, G, RL)
        return out, rk, rv

    def snapshot(self):
        return [x.clone() for x in (*self.full, *self.rfull)]


ALL = [(dt, D, nb) for dt in (torch.bfloat16, torch.float16, torch.float32) for D in (128, 64) for nb in (2, 4, 8)]


# ---- 3. coincident plans are bit-identical ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,nbits", ALL, ids=[f"{str(a[0])[6:]}-D{a[1]}-{a[2]}b" for a in ALL])
def test_coincident_plans_are_bit_identical(kvc, gpu_device, dtype, D, nbits):
    """(Tq, Rr) = (capacity, res_capacity - t): the bound IS the cache, so `out` and the residual are kvc_decode_step_quant's bytes —
    with the four splits of the 232-row setup (t = 1 and 3) and with the single split of a 56-row one."""
    for t, geo in ((1, {}), (3, {}), (3, dict(P=8, qcap=32, rcap=16))):
        st = _State(kvc, gpu_device, dtype, D, nbits, t, seed=nbits + t, **geo)
        st.fill(st.qcap, st.rcap - t).set(st.qcap, st.rcap - t)
        assert (quant_dev_split_plan(1, HQ, t, st.P, st.qcap, st.rcap)[0] > 1) == (not geo)
        want, rk, rv = st.host_step(st.qcap, st.rcap - t)
        got = st.step()
        torch.cuda.synchronize()
        assert torch.isfinite(got.float()).all() and _same(got, want), (t, geo)
        assert _same(st.rk, rk) and _same(st.rv, rv) and _same(st.rk[:, :, st.rcap - t:], st.kn) and _same(st.rv[:, :, st.rcap - t:], st.vn)


# ---- 4. nothing outside the visible rows matters, and the clamps ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,nbits,t,Tq,Rr", [(torch.bfloat16, 128, 4, 1, 64, 23), (torch.float32, 64, 2, 3, 32, 54),
                                                   (torch.float16, 64, 8, 3, 0, 0), (torch.bfloat16, 64, 2, 1, 128, 63),
                                                   (torch.float32, 128, 8, 1, 96, 5)])
def test_nothing_outside_the_visible_rows_matters(kvc, gpu_device, dtype, D, nbits, t, Tq, Rr):
    st = _State(kvc, gpu_device, dtype, D, nbits, t, seed=Tq + Rr, guard=32)
    outs, after = [], []
    for code, meta, row, junk in ((0xFF, float("nan"), float("nan"), float("nan")), (0x00, 3.0e4, -3.0e4, 7.0)):
        st.fill(Tq, Rr, code, meta, row).set(Tq, Rr)
        st.ws.view(torch.float32)[:] = junk
        before = st.snapshot()
        outs.append(st.step().clone())
        now = st.snapshot()
        for x, y in zip(now[:4], before[:4]):                                # the call never writes a quantized segment
            assert _same(x, y)
        g = st.guard
        for x, y, new in zip(now[4:], before[4:], (st.kn, st.vn)):           # the residual: the step's rows, nothing else
            assert _same(x[:, :, :g + Rr], y[:, :, :g + Rr]) and _same(x[:, :, g + Rr + t:], y[:, :, g + Rr + t:])
            assert _same(x[:, :, g + Rr:g + Rr + t], new)
        after.append((st.rk[:, :, :Rr + t].clone(), st.rv[:, :, :Rr + t].clone()))
        assert st.words.tolist() == [Tq, Rr]
    assert torch.isfinite(outs[0].float()).all()
    assert _same(outs[0], outs[1]) and _same(after[0][0], after[1][0]) and _same(after[0][1], after[1][1])


@pytest.mark.parametrize("dtype,D,nbits,t", [(torch.bfloat16, 128, 4, 1), (torch.float32, 64, 2, 3)])
def test_words_are_clamped_to_the_buffers(kvc, gpu_device, dtype, D, nbits, t):
    """-5 and 10^6 in either word behave as the clamped values; the tail and the residual are views between guard rows of a sentinel
    inside one allocation each, and the guards keep every bit."""
    guard = 64
    for wild, clamped in (((-5, 20), (0, 20)), ((10 ** 6, 20), (QCAP, 20)), ((64, -5), (64, 0)), ((64, 10 ** 6), (64, RCAP - t)),
                          ((-5, 10 ** 6), (0, RCAP - t)), ((10 ** 6, -5), (QCAP, 0))):
        res = []
        for tw, rw in (wild, clamped):
            st = _State(kvc, gpu_device, dtype, D, nbits, t, seed=5, guard=guard)
            st.fill(QCAP, RCAP, 0xA5, 12345.0, 12345.0)                      # every row inside the buffers live, the guards a sentinel
            st.set(tw, rw)
            before = st.snapshot()
            out = st.step().clone()
            now = st.snapshot()
            for x, y in zip(now[:4], before[:4]):
                assert _same(x, y)
            for x, y in zip(now[4:], before[4:]):
                assert _same(x[:, :, :guard], y[:, :, :guard]) and _same(x[:, :, guard + RCAP:], y[:, :, guard + RCAP:]), (wild, tw, rw)
            assert st.words.tolist() == [tw, rw]
            res.append((out, st.rk.clone(), st.rv.clone()))
        for x, y in zip(*res):
            assert _same(x, y), wild
        assert torch.isfinite(res[0][0].float()).all()
        assert _same(res[0][1][:, :, clamped[1]:clamped[1] + t], st.kn)


# ---- 5. capture at the entry level ------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_across_split_boundaries_and_a_flush(kvc, gpu_device):
    """One call and the in-graph add on the residual word captured on a side stream; 70 replays from (Tq, Rr) = (0, 20) in the
    232-row setup (visible rows 61 .. 130: two boundaries of the 64-row plan) with fresh q / k / v copied into static buffers.  When
    the residual holds 64 rows they are quantized onto the tail eagerly between two replays and the words are rewritten by device
    ops.  Every replay's out equals an eager call of the same entry on a twin state; tails and residuals end byte-identical.
    Replays and flushes run under sync debug mode "error"."""
    dtype, D, nbits, t, R0, steps = torch.bfloat16, 128, 4, 1, 20, 70
    rps = quant_dev_split_plan(1, HQ, t, P0, QCAP, RCAP)[1]
    assert (P0 + R0 + steps) // rps - (P0 + R0 + t) // rps >= 2              # the visible rows cross two boundaries of the plan
    a, b = (_State(kvc, gpu_device, dtype, D, nbits, t, seed=3).fill(0, R0).set(0, R0) for _ in range(2))
    g = torch.Generator().manual_seed(9)
    feed = [[torch.randn(1, h, t, D, generator=g).to(dtype).to(gpu_device) for h in (HQ, HKV, HKV)] for _ in range(steps)]
    out = torch.empty(1, t, HQ, D, dtype=dtype, device=gpu_device)
    a.step(out)                                                              # warm-up: residual row R0 is rewritten below
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(gpu_device), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        a.step(out)
        a.words[1:2].add_(t)
    torch.cuda.synchronize()
    got, want, mirror, flushes = [], [], [0, R0], 0
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fq, fk, fv in feed:
            a.q.copy_(fq)
            a.kn.copy_(fk)
            a.vn.copy_(fv)
            graph.replay()
            got.append(out.clone())
            want.append(b.step(q=fq, kn=fk, vn=fv))
            b.words[1:2].add_(t)
            mirror[1] += t
            if mirror[1] == RL:                                              # the flush, from the host mirror alone
                for s in (a, b):
                    kvc.quantize_rows(s.rk[:, :, :RL], s.tail[0], s.tail[2], mirror[0], kvc.QUANT_KEYS, nbits, G)
                    kvc.quantize_rows(s.rv[:, :, :RL], s.tail[1], s.tail[3], mirror[0], kvc.QUANT_VALUES, nbits, G)
                    s.words[0:1].add_(RL)
                    s.words[1:2].zero_()
                mirror, flushes = [mirror[0] + RL, 0], flushes + 1
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert flushes == 1 and a.words.tolist() == b.words.tolist() == mirror == [64, R0 + steps - 64]
    for j, (x, y) in enumerate(zip(got, want)):
        assert _same(x, y), f"replay {j}"
    for x, y in zip((*a.tail, a.rk, a.rv), (*b.tail, b.rk, b.rv)):
        assert _same(x[:, :, :64] if x.shape[2] >= 64 else x[:, :, :2], y[:, :, :64] if y.shape[2] >= 64 else y[:, :, :2])
    assert _same(a.rk[:, :, :mirror[1]], b.rk[:, :, :mirror[1]]) and _same(a.rv[:, :, :mirror[1]], b.rv[:, :, :mirror[1]])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
def _config(layers=3):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=4096, intermediate_size=256, num_hidden_layers=layers, num_attention_heads=32, num_key_value_heads=8,
                       head_dim=128, vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa", eos_token_id=None,
                       pad_token_id=0, bos_token_id=None)


class _Model:
    """The other GPU files' tiny Llama with the forwards of `method` patched in (restored on exit)."""

    def __init__(self, method, cap=64, window=8, layers=3, merge=None):
        self.method, self.cap, self.window, self.layers, self.merge = method, cap, window, layers, merge

    def __enter__(self):
        from transformers import LlamaForCausalLM
        from kvcache_factory_amd import monkeypatch as mp
        mp.replace_llama(self.method)
        torch.manual_seed(0)
        model = LlamaForCausalLM(_config(self.layers)).to(torch.bfloat16).to("cuda:0").eval()
        for layer in model.model.layers:
            for name, val in (("window_size", self.window), ("max_capacity_prompt", self.cap), ("kernel_size", 7), ("pooling", "maxpool"),
                              ("merge", self.merge)):
                setattr(layer.self_attn.config, name, val)
        return model

    def __exit__(self, *exc):
        from kvcache_factory_amd import monkeypatch as mp
        mp.replace_llama("fullkv")


def _ids(n, dev, seed=5):
    return torch.randint(1, 256, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


def _decode(dec, ids, steps, watch=False):
    """Greedy: -> (tokens [1, steps], logits of the prefill and of every step, the memory allocated after every replayed step that
    neither captured nor grew, by tail capacity).  Tokens and logits go into buffers made up front."""
    first = dec.prefill(ids)
    logits = torch.empty(steps + 1, *first.shape, dtype=first.dtype, device=first.device)
    toks = torch.empty(first.shape[0], steps, dtype=torch.long, device=first.device)
    logits[0] = first
    mem = collections.defaultdict(list)
    for j in range(steps):
        toks[:, j] = logits[j][:, -1].argmax(-1)
        replay = watch and dec._graph is not None
        if replay:
            torch.cuda.set_sync_debug_mode("error")                          # a replayed step (and its flush) never waits for the device
        try:
            logits[j + 1] = dec.step(toks[:, j:j + 1])
        finally:
            torch.cuda.set_sync_debug_mode(0)
        if replay and dec._graph is not None:
            mem[dec._capacity].append(torch.cuda.memory_allocated())
    return toks, list(logits), mem


def _same_layers(a, b):
    for la, lb in zip(a._cache.layers, b._cache.layers):
        assert la.rows() == lb.rows() and la.get_seq_length() == lb.get_seq_length()
        (pa, ta, ra), (pb, tb, rb) = la.segments(), lb.segments()
        G_ = la.group_size
        for x, y, rows in zip(pa[:4] + ta[:4] + ra[:2], pb[:4] + tb[:4] + rb[:2],
                              (pa[4], pa[4], -(-pa[4] // G_), pa[4], ta[4], ta[4], ta[4] // G_, ta[4], ra[2], ra[2])):
            assert _same(x[:, :, :rows], y[:, :, :rows])


def _replay_equals_eager(method, nbits, steps, seed=5, watch=True, **kw):
    from kvcache_factory_amd import GraphDecoder
    from kvcache_factory_amd.cache import quant_schedule
    ids = _ids(300, "cuda:0", seed)
    with _Model(method) as model:
        a, b = GraphDecoder(model, nbits=nbits, **kw), GraphDecoder(model, nbits=nbits, capture=False, **kw)
        ta, la, mem = _decode(a, ids, steps, watch=watch)
        tb, lb, _ = _decode(b, ids, steps)
        torch.cuda.synchronize()
        flushes, tails, grows, captures = quant_schedule(kw["residual_length"], a.tail_rows, steps)
        assert (a.grows, a.captures, b.grows, b.captures) == (grows, captures, grows, 0)
        assert all(layer.flushes == len(flushes) and layer.rows()[1:] == (tails[-1] if tails else 0, steps - (tails[-1] if tails else 0))
                   for layer in a._cache.layers)
        assert torch.equal(ta, tb)
        for j, (x, y) in enumerate(zip(la, lb)):
            assert _same(x, y), f"step {j}"
        _same_layers(a, b)
        assert a._cache.get_seq_length() == 300 + steps and a._counter[1].tolist() == [steps - (tails[-1] if tails else 0)] * 3
        return a, mem


def test_replay_equals_eager_across_flushes_and_grows(kvc, gpu_device):
    """SnapKV, cap 64, W 8, a 300-token prompt, nbits 4, G 32, R 64, tail_rows 64, 300 greedy tokens: four flushes, two
    grow-and-re-capture events; tokens, every step's logits and every layer's codes, metadata and residual rows in use are
    byte-identical to capture=False; memory is flat between grow events and no replayed step synchronises."""
    a, mem = _replay_equals_eager("snapkv", 4, 300, q_group_size=32, residual_length=64, tail_rows=64)
    assert a._cache.layers[0].flushes >= 4 and a.grows >= 2 and a.captures == a.grows + 1
    assert len(mem) >= 3 and sum(len(v) for v in mem.values()) >= 300 - 2 * a.captures - a.grows
    for cap, seen in mem.items():
        assert len(set(seen)) == 1, f"memory moved between replays at capacity {cap}: {sorted(set(seen))}"


def test_pyramidkv_layers_of_different_prefix_lengths(kvc, gpu_device):
    a, _ = _replay_equals_eager("pyramidkv", 4, 80, seed=6, watch=False, q_group_size=32, residual_length=64, tail_rows=64)
    assert len({layer.rows()[0] for layer in a._cache.layers}) > 1            # the pyramid: every layer its own prefix


@pytest.mark.parametrize("nbits", [2, 8])
def test_two_and_eight_bits(kvc, gpu_device, nbits):
    _replay_equals_eager("snapkv", nbits, 80, seed=7, watch=False, q_group_size=32, residual_length=64, tail_rows=64)


# ---- 7. against the host-issued quantized path --------------------------------------------------------------------------------------------------
def _against_host_issued(layers, steps, check_layers):
    from kvcache_factory_amd import GraphDecoder, QuantizedCompressedCache
    nbits, G_, RL_ = 4, 32, 64
    ids = _ids(300, "cuda:0")
    with _Model("snapkv", layers=layers) as model:
        dec = GraphDecoder(model, nbits=nbits, q_group_size=G_, residual_length=RL_, tail_rows=64)
        toks, logits, _ = _decode(dec, ids, steps)
        cache = QuantizedCompressedCache(model.config, nbits=nbits, q_group_size=G_, residual_length=RL_)
        with torch.no_grad():
            ref = [model(ids, past_key_values=cache, use_cache=True).logits[:, -1:]]
            for j in range(steps):
                ref.append(model(toks[:, j:j + 1], past_key_values=cache, use_cache=True).logits)
        torch.cuda.synchronize()
        assert all(layer._mode == "fused" for layer in cache.layers)         # the host-issued path was the fused one
        for i in check_layers:
            mine, host = dec._cache.layers[i], cache.layers[i]
            pre, qt, (rk, rv, rr) = mine.segments()
            assert (pre[4], qt[4], rr) == (host._prows, host._trows, host._rrows) and qt[4] == steps // RL_ * RL_ and rr == steps % RL_
            for x, y, rows in zip(pre[:4] + qt[:4], (host._pkc, host._pvc, host._pkm, host._pvm, host._tkc, host._tvc, host._tkm, host._tvm),
                                  (pre[4], pre[4], -(-pre[4] // G_), pre[4], qt[4], qt[4], qt[4] // G_, qt[4])):
                assert _same(x[:, :, :rows], y[:, :, :rows]), f"layer {i}"
            assert _same(rk[:, :, :rr], host._rk[:, :, :rr]) and _same(rv[:, :, :rr], host._rv[:, :, :rr])
        worst = 0.0
        for x, y in zip(logits, ref):
            worst = max(worst, float((x.float() - y.float()).abs().max()) / float(y.float().abs().max()))
        return worst


def test_bytes_and_logits_of_the_host_issued_path_one_layer(kvc, gpu_device):
    """A 1-layer model (the layer's K / V depend on the token embeddings only): after 150 replayed steps the prefix codes and metadata,
    the tail rows in use and the residual rows in use are byte-identical to QuantizedCompressedCache's teacher-forced with the same
    tokens — the flush schedule and the quantize calls are the host-issued path's —, and every step's logits are within 3 % of the
    largest logit (the project's bound for two attention kernels over the same cache bytes: the split plans differ)."""
    worst = _against_host_issued(1, 150, (0,))
    print(f"replayed vs host-issued quantized path, 1 layer: worst |logit diff| / max |logit| = {worst:.4f} over 151 steps")
    assert worst <= 3e-2


def test_bytes_of_layer_zero_three_layers(kvc, gpu_device):
    """Three layers: layer 0's bytes as above; deeper layers see rounding-different inputs, so only the logit ratio is printed."""
    worst = _against_host_issued(3, 150, (0,))
    print(f"replayed vs host-issued quantized path, 3 layers: worst |logit diff| / max |logit| = {worst:.4f} over 151 steps")


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_anything_is_stored(kvc, gpu_device):
    from transformers import DynamicCache
    from kvcache_factory_amd import GraphDecoder, KVQuantCompressedCache, QuantizedCompressedCache
    ids = _ids(100, gpu_device)
    with _Model("snapkv") as model:
        for kw, msg in ((dict(nbits=3), "nbits"), (dict(nbits=4, q_group_size=48), "q_group_size"),
                        (dict(nbits=4, q_group_size=64, residual_length=96), "residual_length"),
                        (dict(nbits=4, interval=8), "not both"), (dict(nbits=4, heavy_hitter=8), "not both")):
            with pytest.raises(ValueError, match=msg):
                GraphDecoder(model, **kw)
        dec = GraphDecoder(model, nbits=4, q_group_size=32, residual_length=64, tail_rows=64)
        plain = DynamicCache(config=model.config)
        with pytest.raises(ValueError, match="past_key_values"):
            dec.prefill(ids, past_key_values=plain)
        assert plain.get_seq_length() == 0
        with pytest.raises(NotImplementedError, match="one sequence"):
            dec.prefill(torch.cat([ids, ids]))
        for cache in (QuantizedCompressedCache(model.config, nbits=4), KVQuantCompressedCache(model.config, nbits=4)):
            with pytest.raises(NotImplementedError, match="quantized"):
                dec.prefill(ids, past_key_values=cache)
            assert all(layer.get_seq_length() == 0 for layer in cache.layers)
        assert dec._cache is None and dec._graph is None and dec.captures == 0
    for method in ("adakv", "headkv", "think"):
        with _Model(method) as model:
            with pytest.raises(NotImplementedError, match=method):
                GraphDecoder(model, nbits=4)
    with _Model("snapkv", merge="pivot") as model:
        with pytest.raises(NotImplementedError, match="merge"):
            GraphDecoder(model, nbits=4)
