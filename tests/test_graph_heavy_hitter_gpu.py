"""Heavy-hitter eviction under graph-replayed decoding on the MI355X.

The entry (kvc_decode_step_dev_scored): the scored specs of the conformance harness (tests/decode_ref.py) through an adapter that
embeds each case's tail and its scores in NaN-filled buffers of `capacity` rows and puts the lengths into device words (needles
row-exact with their scores, the per-element bound at the harness's factor 4); one step's scores against fp64 within 4 x the fp32
restatement's own error; the edges — a prefix word below the buffers' rows, an empty tail under a multi-split bound, a step that
crosses a split boundary, wild counter values between guard rows — with `out` bit-identical to kvc_decode_step_dev everywhere and,
at the full bound, `out` and scores bit-identical to kvc_decode_step_scored; a captured call replayed across a split boundary.
The layer (BoundedHeavyHitterLayer) beside HeavyHitterLayer on the same rows, every eviction exact from its own state in both tie
modes.  End to end (GraphDecoder(model, heavy_hitter=8) on the tiny Llama / Mistral of the other GPU files): replay == capture=False
bit for bit over 240 tokens, one capture, flat memory, no host synchronisation, bounded rows."""
import collections

import pytest
import torch

import decode_ref as DR
import heavy_hitter_ref as R
from test_decode_conformance_cpu import run_bound, run_needles
from test_graph_decode_cpu import dev_split_plan
from test_graph_heavy_hitter_cpu import CAPS, SCORED, scored_adapter

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- 1. conformance through the existing harness ------------------------------------------------------------------------------------------
CONF = [(s, c) for s in SCORED for c in CAPS]
CONF_IDS = [f"{DR.spec_id(s)}-{c}" for s, c in CONF]


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_needles_row_exact(kvc, gpu_device, spec, cap):
    seen = []
    probes = run_needles(spec, scored_adapter(kvc.decode_step_dev_scored, CAPS[cap], seen), gpu_device)      # check_scores included
    assert cap == "own" or min(seen) > 1                                     # the wide bound really ran split
    print(f"{DR.spec_id(spec)} ({cap}, {max(seen)} splits): {probes} needles returned their row and took their score")


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_per_element_bound(kvc, gpu_device, spec, cap):
    e_kernel, e_ref = run_bound(spec, scored_adapter(kvc.decode_step_dev_scored, CAPS[cap]), gpu_device)
    key = str(spec["dtype"])[6:]
    RATIOS[key] = max(RATIOS[key], e_kernel / e_ref)
    print(f"{DR.spec_id(spec)} ({cap}): e_kernel / e_ref = {e_kernel / e_ref:.3f} (e_ref = {e_ref:.3e})")


def test_report_ratios():
    """The largest e_kernel / e_ref per dtype of this run (the bound allows 4)."""
    for dt, r in sorted(RATIOS.items()):
        print(f"e_kernel / e_ref  dev_scored {dt:9s} {r:.3f}")
        assert r <= DR.FACTOR


# ---- direct calls ---------------------------------------------------------------------------------------------------------------------------
HQ = 8


def _state(dev, dtype, D, G, t, pcap, cap, seed=0, guard=0, fill=float("nan")):
    """A layer's buffers before a step of t tokens: unit-variance K, queries of standard deviation 1.5, every row and score slot live
    (callers poison what must not be seen).  The tail K / V / scores are VIEWS between `guard` rows of `fill` on both sides."""
    g = torch.Generator().manual_seed(seed)
    hkv = HQ // G
    mk = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dtype).to(dev)      # noqa: E731
    c = dict(q=mk(1, HQ, t, D, s=1.5), kn=mk(1, hkv, t, D), vn=mk(1, hkv, t, D), kp=mk(1, HQ, pcap, D), vp=mk(1, HQ, pcap, D),
             pcap=pcap, cap=cap, t=t, G=G, scaling=D ** -0.5, guard=guard)
    c["kfull"] = torch.full((1, hkv, guard + cap + guard, D), fill, dtype=dtype, device=dev)
    c["vfull"] = torch.full_like(c["kfull"], fill)
    c["sfull"] = torch.full((1, HQ, guard + cap + guard), fill, dtype=torch.float32, device=dev)
    c["kt"], c["vt"], c["st"] = (c[n][:, :, guard:guard + cap] for n in ("kfull", "vfull", "sfull"))
    c["kt"].copy_(mk(1, hkv, cap, D))
    c["vt"].copy_(mk(1, hkv, cap, D))
    c["st"].copy_((torch.rand(1, HQ, cap, generator=g) * 10).to(dev))
    c["sp"] = (torch.rand(1, HQ, pcap, generator=g) * 10).to(dev)
    return c


def _clone(c):
    d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c.items()}
    g = d["guard"]
    d["kt"], d["vt"], d["st"] = (d[n][:, :, g:g + d["cap"]] for n in ("kfull", "vfull", "sfull"))
    return d


def _words(dev, T, P=None):
    return torch.tensor([T], dtype=torch.int32, device=dev), (None if P is None else torch.tensor([P], dtype=torch.int32, device=dev))


def _scored_ws(kvc, c, fill=None):
    n = kvc.decode_dev_scored_plan(c["q"], c["kn"], c["kp"], c["pcap"], c["kt"], c["sp"], c["st"])[1]
    ws = torch.empty(n + 256, dtype=torch.uint8, device=c["q"].device)
    if fill is not None:
        ws.view(torch.float32)[:] = fill
    return ws


def _dev_scored(kvc, c, counter, rows_b, ws=None, out=None):
    return kvc.decode_step_dev_scored(c["q"], c["kn"], c["vn"], c["kp"], c["vp"], c["pcap"], c["kt"], c["vt"], counter, c["sp"], c["st"],
                                      c["scaling"], rows_b=rows_b, ws=ws, out=out)


def _dev(kvc, c, counter, rows_b):
    """kvc_decode_step_dev with the same arguments and its full workspace."""
    n = kvc.decode_dev_plan(c["q"], c["kn"], c["kp"], c["pcap"], c["kt"])[1]
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=c["q"].device)
    return kvc.decode_step_dev(c["q"], c["kn"], c["vn"], c["kp"], c["vp"], c["pcap"], c["kt"], c["vt"], counter, c["scaling"], rows_b=rows_b,
                               ws=ws)


def _scores(c, P, rows):
    return torch.cat([c["sp"][:, :, :P], c["st"][:, :, :rows - P]], 2)


# ---- 2. one step against fp64 -------------------------------------------------------------------------------------------------------------
STEP = [(dt, D, G, t, PB) for dt in (torch.bfloat16, torch.float16) for D in (64, 128) for G in (1, 4) for t in (1, 3)
        for PB in ((40, 51), (500, 702))]                                     # (prefix rows, bound rows): one split, several


@pytest.mark.parametrize("dtype,D,G,t,PB", STEP, ids=[f"{str(s[0])[6:]}-D{s[1]}-G{s[2]}-t{s[3]}-P{s[4][0]}bound{s[4][1]}" for s in STEP])
def test_scored_step_against_fp64(kvc, gpu_device, dtype, D, G, t, PB):
    """The step at the full bound (T + t == capacity, the prefix word at prefix_rows): the scores of one step against fp64 — kernel
    error <= 4 x the fp32 torch restatement's on the same tensors, from zero and from known scores with junk where the step's own
    rows go — and, the two split plans being the same, `out` and every score bit-identical to kvc_decode_step_scored; `out`
    bit-identical to kvc_decode_step_dev."""
    P, bound = PB
    cap = bound - P
    T = cap - t
    assert dev_split_plan(1, HQ, t, P, cap) == DR.split_plan(1, HQ, t, P + T + t) and (dev_split_plan(1, HQ, t, P, cap)[0] > 1) == (bound > 64)
    c = _state(gpu_device, dtype, D, G, t, P, cap, seed=P + D + G + t)
    counter, rows_b = _words(gpu_device, T, P)
    zero = _clone(c)
    zero["sp"].zero_()
    zero["st"].zero_()
    out = _dev_scored(kvc, zero, counter, rows_b)
    p64, e_ref = R.one_step_bound(zero["q"], zero["kp"], zero["kt"], P, T, zero["scaling"])
    e_kernel = R.max_rel_err(_scores(zero, P, bound), R.step_increment(p64, bound))
    print(f"one-step max relative error: kernel {e_kernel:.3e}, fp32 torch {e_ref:.3e}")
    assert e_kernel <= 4 * e_ref, (e_kernel, e_ref)
    d = _clone(c)
    d["st"][:, :, T:] = 123.0                                                 # junk where the step's own rows will be
    before = _scores(d, P, bound).clone()
    out_d = _dev_scored(kvc, d, counter, rows_b)
    R.check_step(before, _scores(d, P, bound), p64, e_ref, P + T)
    # the host-counted entry on the same state: same plan, same bytes
    h = _clone(c)
    h["st"][:, :, T:] = 123.0
    out_h = kvc.decode_step_scored(h["q"], h["kn"], h["vn"], h["kp"], h["vp"], P, h["kt"], h["vt"], T, h["sp"], h["st"], h["scaling"])
    assert torch.equal(_bits(out_d), _bits(out_h)) and torch.equal(_bits(out), _bits(out_h))
    assert torch.equal(_bits(d["sp"]), _bits(h["sp"])) and torch.equal(_bits(d["st"]), _bits(h["st"]))
    assert torch.equal(_bits(d["kt"]), _bits(h["kt"])) and torch.equal(_bits(d["vt"]), _bits(h["vt"]))
    assert torch.equal(_bits(_dev(kvc, _clone(c), counter, rows_b)), _bits(out))


# ---- 3. edges (hq 8, hkv 2, Pcap 64, cap 24: a bound of 88 rows, two splits of 64) --------------------------------------------------------------
PCAP, TCAP = 64, 24
# (prefix word, counter, t): the word below the buffers' rows; an empty tail whose trailing split is empty; steps whose tokens sit
# on both sides of the boundary at 64 rows; the full bound
EDGES = [(40, 5, 1), (40, 0, 1), (40, 0, 3), (42, 21, 3), (None, 0, 1), (64, 0, 3), (40, 23, 1), (64, 21, 3), (None, 23, 1), (0, 7, 3)]


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 64), (torch.float32, 64)])
@pytest.mark.parametrize("Pw,T,t", EDGES, ids=[f"P{e[0]}-T{e[1]}-t{e[2]}" for e in EDGES])
def test_edges(kvc, gpu_device, dtype, D, Pw, T, t):
    """Everything behind the visible rows — prefix rows and score slots [P_b, 64), tail rows and score slots at or past T + t, the
    workspace — is NaN before the call: the result is finite, those slots are still NaN, the tail maps to virtual rows r - P_b (the
    scores against fp64 at (P_b, T)), `out` is kvc_decode_step_dev's and, at the full bound, everything is kvc_decode_step_scored's."""
    assert dev_split_plan(1, HQ, t, PCAP, TCAP) == (2, 64)
    P = PCAP if Pw is None else Pw
    assert T + t <= TCAP                                                     # (no clamp here: test_counter_is_clamped_between_guard_rows)
    rows, nan = P + T + t, float("nan")
    c = _state(gpu_device, dtype, D, 4, t, PCAP, TCAP, seed=7 + rows)
    for name, lo in (("kp", P), ("vp", P), ("sp", P), ("kt", T), ("vt", T), ("st", T)):
        c[name][:, :, lo:] = nan                                              # (the step's own slots included: they start from 0)
    ref = _clone(c)
    counter, rows_b = _words(gpu_device, T, Pw)
    before = torch.zeros(1, HQ, rows, dtype=torch.float32, device=gpu_device)
    before[:, :, :P + T] = _scores(c, P, P + T)
    out = _dev_scored(kvc, c, counter, rows_b, ws=_scored_ws(kvc, c, fill=nan))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(_scores(c, P, rows)).all()
    for name, lo in (("kp", P), ("vp", P), ("sp", P), ("kt", T + t), ("vt", T + t), ("st", T + t)):
        assert bool(torch.isnan(c[name][:, :, lo:].float()).all()), name
    assert torch.equal(_bits(c["kt"][:, :, T:T + t]), _bits(c["kn"])) and torch.equal(_bits(c["vt"][:, :, T:T + t]), _bits(c["vn"]))
    assert torch.equal(_bits(c["kt"][:, :, :T]), _bits(ref["kt"][:, :, :T])) and torch.equal(_bits(c["kp"][:, :, :P]), _bits(ref["kp"][:, :, :P]))
    assert int(counter) == T and (rows_b is None or int(rows_b) == Pw)
    p64, e_ref = R.one_step_bound(c["q"], c["kp"], c["kt"], P, T, c["scaling"])
    R.check_step(before, _scores(c, P, rows), p64, e_ref, P + T)
    assert torch.equal(_bits(_dev(kvc, ref, counter, rows_b)), _bits(out))
    if P == PCAP and T + t == TCAP:                                          # the full bound: the host-counted entry's plan
        assert DR.split_plan(1, HQ, t, rows) == (2, 64)
        h = _clone(ref)
        h["kt"][:, :, T:], h["vt"][:, :, T:] = 0, 0                           # (that entry's own checks want nothing; keep NaN out of its sight)
        out_h = kvc.decode_step_scored(h["q"], h["kn"], h["vn"], h["kp"], h["vp"], P, h["kt"], h["vt"], T, h["sp"], h["st"], h["scaling"])
        assert torch.equal(_bits(out), _bits(out_h))
        assert torch.equal(_bits(c["sp"]), _bits(h["sp"])) and torch.equal(_bits(c["st"]), _bits(h["st"]))


@pytest.mark.parametrize("dtype,D,t", [(torch.bfloat16, 128, 1), (torch.float32, 64, 3)])
def test_counter_is_clamped_between_guard_rows(kvc, gpu_device, dtype, D, t):
    """Counter values -5 and capacity + 100 with the tail K / V / scores views between 100 + t + 28 guard rows of a sentinel on both
    sides: the guards keep every bit, output and scores equal the call with the clamped value."""
    guard, sentinel = 100 + t + 28, 12345.0
    for wild, clamped in ((-5, 0), (TCAP + 100, TCAP - t)):
        res = []
        for value in (wild, clamped):
            c = _state(gpu_device, dtype, D, 4, t, PCAP, TCAP, seed=11, guard=guard, fill=sentinel)
            counter, rows_b = _words(gpu_device, value, 40)
            out = _dev_scored(kvc, c, counter, rows_b)
            torch.cuda.synchronize()
            for full in (c["kfull"], c["vfull"], c["sfull"]):
                assert (full[:, :, :guard] == sentinel).all() and (full[:, :, guard + TCAP:] == sentinel).all(), (wild, value)
            assert int(counter) == value
            res.append((out.clone(), c["kt"].clone(), c["vt"].clone(), c["st"].clone(), c["sp"].clone()))
        for x, y in zip(*res):
            assert torch.equal(_bits(x), _bits(y)), wild
        assert torch.equal(_bits(res[0][1][:, :, clamped:clamped + t]), _bits(c["kn"]))


# ---- 4. a captured call ------------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_across_a_split_boundary(kvc, gpu_device):
    """One call and the in-graph counter add_ captured on a side stream; 14 replays from T = 10 with a prefix word of 48 in the
    (64, 24) setup (visible rows 59 .. 72: over the boundary of the 64-row plan) with fresh q / k / v copied into static buffers.
    Every replay's out and the scores after it equal an eager call of the same entry on a copy of the state, bit for bit.  Replays
    run under sync debug mode "error"."""
    dtype, D, t, P, T0, steps = torch.bfloat16, 128, 1, 48, 10, 14
    assert dev_split_plan(1, HQ, t, PCAP, TCAP) == (2, 64) and P + T0 + t < 64 < P + T0 + steps
    c = _state(gpu_device, dtype, D, 4, t, PCAP, TCAP, seed=3)
    e = _clone(c)                                                            # the eager twin's state
    g = torch.Generator().manual_seed(9)
    feed = [[(torch.randn(1, h, t, D, generator=g) * s).to(dtype).to(gpu_device) for h, s in ((HQ, 1.5), (2, 1.0), (2, 1.0))] for _ in range(steps)]
    counter, rows_b = _words(gpu_device, T0, P)
    ecounter = counter.clone()
    ws, ews = _scored_ws(kvc, c), _scored_ws(kvc, c)
    out = torch.empty(1, t, HQ, D, dtype=dtype, device=gpu_device)
    kept = c["sp"].clone(), c["st"].clone()
    _dev_scored(kvc, c, counter, rows_b, ws=ws, out=out)                      # warm-up: row T0 is rewritten below, the scores put back
    c["sp"].copy_(kept[0])
    c["st"].copy_(kept[1])
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(gpu_device), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _dev_scored(kvc, c, counter, rows_b, ws=ws, out=out)
        counter.add_(t)
    torch.cuda.synchronize()
    got, want = [], []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fq, fk, fv in feed:
            c["q"].copy_(fq)
            c["kn"].copy_(fk)
            c["vn"].copy_(fv)
            graph.replay()
            got.append((out.clone(), c["sp"].clone(), c["st"].clone()))
            e["q"], e["kn"], e["vn"] = fq, fk, fv
            want.append((_dev_scored(kvc, e, ecounter, rows_b, ws=ews), e["sp"].clone(), e["st"].clone()))
            ecounter.add_(t)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert int(counter) == int(ecounter) == T0 + steps
    for j, (x, y) in enumerate(zip(got, want)):
        n = T0 + j + 1
        assert torch.equal(_bits(x[0]), _bits(y[0])), f"replay {j} (T = {T0 + j}): out"
        assert torch.equal(_bits(x[1][:, :, :P]), _bits(y[1][:, :, :P])) and torch.equal(_bits(x[2][:, :, :n]), _bits(y[2][:, :, :n])), f"replay {j}: scores"
    assert torch.equal(_bits(c["kt"]), _bits(e["kt"])) and torch.equal(_bits(c["vt"]), _bits(e["vt"]))
    assert torch.equal(_bits(c["sp"]), _bits(e["sp"])) and torch.equal(_bits(c["st"]), _bits(e["st"]))


# ---- 5. the layer beside the host-counted one ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", ["torch_cpu", "canonical"])
@pytest.mark.parametrize("P0", [28, 48])
def test_bounded_layer_beside_the_host_counted_layer(kvc, gpu_device, monkeypatch, P0, tie):
    """50 one-token steps (P0 = 28: 52, as many as the second eviction needs) of both layers on the same rows: the same eviction steps;
    the scores of both within check_step's bound of fp64 at every step, each from its own rows; every eviction of the bounded layer
    equal to heavy_hitter_ref.evict_reference on its own K, V and scores read back just before it, bit for bit."""
    from kvcache_factory_amd import BoundedHeavyHitterLayer, HeavyHitterLayer, pyramidkv_utils as pu
    monkeypatch.setattr(pu, "TIE_MODE", tie)
    hq, hkv, D, B, W, interval, dt = 8, 2, 64, 48, 8, 16, torch.bfloat16
    cl = pu.H2OKVCluster(window_size=W, max_capacity_prompt=B)
    g = torch.Generator().manual_seed(P0)
    mk = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dt).to(gpu_device)      # noqa: E731
    k0, v0, s0 = mk(1, hq, P0, D), mk(1, hq, P0, D), (torch.rand(1, hq, P0, generator=g) * 3).to(gpu_device)
    host, seed = HeavyHitterLayer(interval), HeavyHitterLayer(interval)
    for x in (host, seed):
        x.prefill(k0.clone(), v0.clone(), 500)
        x._sbuf[:, :, :P0] = s0
    counters = torch.full((3,), 77, dtype=torch.int32, device=gpu_device)
    layer = BoundedHeavyHitterLayer.adopt(seed, cl, interval, counters[1:2], hkv)
    addresses = [x.data_ptr() for x in (layer._kbuf, layer._vbuf, layer._sbuf, layer._ktail, layer._vtail, layer._stail, layer._dev_ws)]
    at = []
    for step in range(52 if P0 < B else 50):
        q, k, v = mk(1, hq, 1, D, s=1.5), mk(1, hkv, 1, D), mk(1, hkv, 1, D)
        for x in (host, layer):
            P, T = x.rows()
            before = torch.zeros(1, hq, P + T + 1, dtype=torch.float32, device=gpu_device)
            before[:, :, :P + T] = x.scores()
            x.decode_attend(q, k, v, D ** -0.5)
            if x is layer:
                counters[1:2].add_(1)
                layer.advance(1)
            p64, e_ref = R.one_step_bound(q, x._kbuf, x._ktail, P, T, D ** -0.5)
            R.check_step(before, x.scores(), p64, e_ref, P + T)
        n0 = host.evictions
        host.after_decode(cl, q)
        layer.after_decode(cl, q)                                            # nothing: the owner calls the trigger
        K, V, score = layer.keys.clone(), layer.values.clone(), layer.scores()
        did = layer.maybe_evict()
        assert did == (host.evictions > n0) and layer.rows() == host.rows() and layer.evictions == host.evictions, step
        assert int(layer._plen) == layer._stored and counters.tolist() == [77, layer._tail, 77]
        assert layer.get_seq_length() == host.get_seq_length() == 501 + step and layer.stored_length() <= B + interval
        if did:
            at.append(step)
            ko, vo, so, _ = R.evict_reference(K, V, score, W, B - W, tie)
            assert layer.rows() == (B, 0)
            assert torch.equal(_bits(layer.keys.cpu()), _bits(ko)) and torch.equal(_bits(layer.values.cpu()), _bits(vo)), step
            assert torch.equal(_bits(layer.scores().cpu()), _bits(so)), step
    assert len(at) >= 2 and at[0] == max(W, B + interval - P0) - 1 and at[1] - at[0] == interval
    assert addresses == [x.data_ptr() for x in (layer._kbuf, layer._vbuf, layer._sbuf, layer._ktail, layer._vtail, layer._stail, layer._dev_ws)]


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------------
class _Model:
    """The other GPU files' tiny 3-layer model with the h2o forwards patched in (restored on exit)."""

    def __init__(self, kind, cap=64, window=8):
        self.kind, self.cap, self.window = kind, cap, window

    def _replace(self):
        from kvcache_factory_amd import monkeypatch as mp
        return mp.replace_llama if self.kind == "llama" else mp.replace_mistral

    def __enter__(self):
        from transformers import LlamaConfig, LlamaForCausalLM, MistralConfig, MistralForCausalLM
        cfg_cls, cls, extra = (LlamaConfig, LlamaForCausalLM, {}) if self.kind == "llama" else (MistralConfig, MistralForCausalLM, dict(sliding_window=None))
        self._replace()("h2o")
        torch.manual_seed(0)
        cfg = cfg_cls(hidden_size=4096, intermediate_size=256, num_hidden_layers=3, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
                      vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa", eos_token_id=None, pad_token_id=0,
                      bos_token_id=None, **extra)
        model = cls(cfg).to(torch.bfloat16).to("cuda:0").eval()
        for layer in model.model.layers:
            for name, val in (("window_size", self.window), ("max_capacity_prompt", self.cap)):
                setattr(layer.self_attn.config, name, val)
        return model

    def __exit__(self, *exc):
        self._replace()("fullkv")


@pytest.mark.parametrize("kind", ["llama", "mistral"])
def test_replayed_generation_with_heavy_hitter_eviction(kvc, gpu_device, kind):
    """L 300, cap 64, W 8, heavy_hitter 8, 240 new tokens, the replayed decoder and capture=False in lockstep: identical tokens and
    logits at every step and identical K / V / score bytes at the end, one capture, no growth, at most B + interval rows stored, flat
    memory once every layer has evicted; then 20 more replayed steps (two evictions per layer among them) under sync debug mode
    "error"."""
    from kvcache_factory_amd import BoundedHeavyHitterLayer, GraphDecoder
    L, cap, W, N, new = 300, 64, 8, 8, 240
    ids = torch.randint(0, 256, (1, L), generator=torch.Generator().manual_seed(3)).to(gpu_device)
    with _Model(kind, cap, W) as model:
        replay, eager = GraphDecoder(model, heavy_hitter=N), GraphDecoder(model, heavy_hitter=N, capture=False)
        le, lr = eager.prefill(ids).clone(), replay.prefill(ids).clone()
        assert torch.equal(_bits(le), _bits(lr))
        for dec in (replay, eager):
            assert all(type(x) is BoundedHeavyHitterLayer and x.rows() == (cap, 0) for x in dec._cache.layers)
            for x in dec._layers:                                            # the prompt's column sums came along
                s = x.scores()
                assert bool((s[:, :, :cap - W] > 0).all()) and float(s[:, :, cap - W:].abs().sum()) == 0
        tok = torch.empty(1, 1, dtype=torch.long, device=gpu_device)
        toks = torch.empty(2, new - 1, dtype=torch.long, device=gpu_device)   # made up front: the loop allocates nothing that stays
        mems = []
        for j in range(new - 1):
            toks[0, j], toks[1, j] = le[0, -1].argmax(-1), lr[0, -1].argmax(-1)
            tok.copy_(toks[0, j])
            le = eager.step(tok)                                             # (the static buffers: compared before the next step)
            lr = replay.step(tok)
            assert torch.equal(_bits(le), _bits(lr)), f"step {j}"
            assert all(x.stored_length() <= cap + N for x in replay._layers + eager._layers)
            if all(x.evictions >= 1 for x in replay._layers + eager._layers):
                torch.cuda.synchronize()
                mems.append(torch.cuda.memory_allocated())
        assert torch.equal(toks[0], toks[1])
        assert replay.captures == 1 and replay.grows == 0 and eager.captures == 0 and eager.grows == 0
        for dec in (replay, eager):
            for layer in dec._layers:
                assert layer.evictions == (new - 1) // N and layer.get_seq_length() == L + new - 1
                assert int(layer._plen) == layer._stored and int(layer._dev_counter) == layer._tail
        for a, b in zip(replay._layers, eager._layers):
            assert a.rows() == b.rows()
            assert torch.equal(_bits(a.keys), _bits(b.keys)) and torch.equal(_bits(a.values), _bits(b.values))
            assert torch.equal(_bits(a.scores()), _bits(b.scores()))
        assert len(mems) >= new - 2 * N and len(set(mems)) == 1, sorted(set(mems))
        assert replay._cache.get_seq_length() == L + new - 1 and replay._pos.tolist() == [[L + new - 1]]
        # replays and evictions of every layer without a host synchronisation, memory still flat
        n0 = [x.evictions for x in replay._layers]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(2 * N + W // 2):
                replay.step(tok)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        assert all(x.evictions >= n + 2 for x, n in zip(replay._layers, n0))
        assert torch.cuda.memory_allocated() == mems[-1] and replay.captures == 1 and replay.grows == 0
