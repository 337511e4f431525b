"""Graph-replayed decoding on the MI355X.

The entry (kvc_decode_step_dev): the conformance harness of tests/decode_ref.py through an adapter that embeds each case's tail in a
NaN-filled buffer of `capacity` rows and puts its length into a device counter (needles bit for bit, the per-element bound at the
harness's factor 4), the split edges of the bound-sized plan, nothing outside the visible rows matters, the clamp of the counter
between guard rows, and a captured call replayed across two split boundaries against eager calls.
End to end (GraphDecoder on the tiny Llama / Mistral of the other GPU files): replay == eager bit for bit across grow-and-re-capture
events, agreement with today's host-counted path, flat memory and no host synchronisation during replays, PyramidKV, a left-padded
batch, the refusals."""
import collections

import pytest
import torch

import decode_ref as R
from test_decode_conformance_cpu import run_bound, run_needles
from test_graph_decode_cpu import dev_split_plan, visible_edges

pytestmark = pytest.mark.gpu

BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
RATIOS = collections.defaultdict(float)


def _bits(t):
    return t.contiguous().view(BITS[t.dtype])


# ---- the adapter: the old entries' signatures over kvc_decode_step_dev ------------------------------------------------------------------
def adapter(kvc, entry, capacity_of, seen=None):
    """fn with decode_step's (entry "step2") or decode_step_rows' ("rows") signature: the case's tail rows [0, T) go into NaN-filled
    buffers of capacity_of(T, t) rows, T into a device counter; after the call the rows [0, T + t) are copied back into the case's
    buffers (which the harness then compares byte for byte) and everything behind them must still be NaN."""
    def run(q, kn, vn, kp, vp, rows_b, P, kt, vt, T, scaling):
        b, hkv, _, D = kt.shape
        t = q.shape[2]
        cap = capacity_of(T, t)
        bk = torch.full((b, hkv, cap, D), float("nan"), dtype=kt.dtype, device=kt.device)
        bv = torch.full_like(bk, float("nan"))
        bk[:, :, :T], bv[:, :, :T] = kt[:, :, :T], vt[:, :, :T]
        counter = torch.tensor([T], dtype=torch.int32, device=kt.device)
        out = kvc.decode_step_dev(q, kn, vn, kp, vp, P, bk, bv, counter, scaling, rows_b=rows_b)
        kt[:, :, :T + t], vt[:, :, :T + t] = bk[:, :, :T + t], bv[:, :, :T + t]
        assert torch.isnan(bk[:, :, T + t:].float()).all() and torch.isnan(bv[:, :, T + t:].float()).all()
        assert int(counter) == T                                             # the library only reads it
        if seen is not None:
            seen.append(dev_split_plan(b, q.shape[1], t, P, cap)[0])
        return out
    if entry == "rows":
        return lambda q, kn, vn, kp, vp, rows_b, P, kt, vt, T, s: run(q, kn, vn, kp, vp, rows_b, P, kt, vt, T, s)
    return lambda q, kn, vn, kp, vp, P, kt, vt, T, s: run(q, kn, vn, kp, vp, None, P, kt, vt, T, s)


# ---- 1. conformance through the existing harness ------------------------------------------------------------------------------------------
SPECS = [s for s in R.GRID if (s["entry"] == "step2" and not s.get("P1")) or s["entry"] == "rows"]
CAPS = {"own": lambda T, t: T + t, "wide": lambda T, t: T + t + 1024}       # the case's own rows; a bound that forces several splits
CONF = [(s, c) for s in SPECS for c in CAPS]
CONF_IDS = [f"{R.spec_id(s)}-{c}" for s, c in CONF]


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_needles_row_exact(kvc, gpu_device, spec, cap):
    seen = []
    probes = run_needles(spec, adapter(kvc, spec["entry"], CAPS[cap], seen), gpu_device)
    assert cap == "own" or min(seen) > 1                                     # the wide bound really ran split
    print(f"{R.spec_id(spec)} ({cap}, {max(seen)} splits): {probes} needles returned their row")


@pytest.mark.parametrize("spec,cap", CONF, ids=CONF_IDS)
def test_conformance_per_element_bound(kvc, gpu_device, spec, cap):
    e_kernel, e_ref = run_bound(spec, adapter(kvc, spec["entry"], CAPS[cap]), gpu_device)
    key = str(spec["dtype"])[6:]
    RATIOS[key] = max(RATIOS[key], e_kernel / e_ref)
    print(f"{R.spec_id(spec)} ({cap}): e_kernel / e_ref = {e_kernel / e_ref:.3f} (e_ref = {e_ref:.3e})")


def test_report_ratios():
    """The largest e_kernel / e_ref per dtype of this run (the bound allows 4; DESIGN.md section 4 records them)."""
    for dt, r in sorted(RATIOS.items()):
        print(f"e_kernel / e_ref  dev     {dt:9s} {r:.3f}")
        assert r <= R.FACTOR


# ---- 2. split edges ---------------------------------------------------------------------------------------------------------------------------
HQ, HKV, P0, CAP = 8, 2, 40, 216
ROWS3 = [40, 0, 17]


def _edges(b, t):
    """Tail lengths at which some batch row's last token sits one row below, at and one row above a boundary of the restated plan."""
    out = set()
    for p in ([P0] if b == 1 else ROWS3):
        splits, rps = dev_split_plan(b, HQ, t, P0, CAP)
        out |= {0, CAP - t}
        for s in range(1, splits):
            out |= {v - p - t for v in (s * rps - 1, s * rps, s * rps + 1) if 0 <= v - p - t <= CAP - t}
    return sorted(out)


EDGE = [(dt, D, b, t, T) for dt in (torch.bfloat16, torch.float32) for D in (128, 64) for b in (1, 3) for t in (1, 3) for T in _edges(b, t)]


def test_edge_set_is_the_plan_s():
    assert dev_split_plan(1, HQ, 1, P0, CAP)[0] >= 4 and dev_split_plan(3, HQ, 3, P0, CAP)[0] >= 2
    assert _edges(1, 1) == visible_edges(1, HQ, 1, P0, CAP)
    assert {0, 22, 23, 24, 87, 88, 215} <= set(_edges(1, 1)) and _edges(1, 3)[-1] == CAP - 3


@pytest.mark.parametrize("dtype,D,b,t,T", EDGE, ids=[f"{str(e[0])[6:]}-D{e[1]}-b{e[2]}-t{e[3]}-T{e[4]}" for e in EDGE])
def test_split_edges(kvc, gpu_device, dtype, D, b, t, T):
    """fp64 attention under the harness bound and every row as a needle, at the tail lengths where the number of splits that run
    changes (capacity 216 whatever T is: the plan is the bound's)."""
    spec = dict(entry="step2" if b == 1 else "rows", dtype=dtype, D=D, hq=HQ, hkv=HKV, b=b, t=t, P=P0 if b == 1 else ROWS3, T=T)
    fn = adapter(kvc, spec["entry"], lambda T_, t_: CAP)
    assert run_needles(spec, fn, gpu_device) >= T + t
    e_kernel, e_ref = run_bound(spec, fn, gpu_device)
    print(f"T={T}: e_kernel / e_ref = {e_kernel / e_ref:.3f}")


# ---- direct calls -------------------------------------------------------------------------------------------------------------------------------
def _state(dev, dtype, D, b, t, seed=0, guard=0, cap=CAP, fill=float("nan")):
    """q, k_new, v_new, prefix [b, HQ, P0 + 5, D], and a tail [b, HKV, cap, D] that is a VIEW into a larger allocation with `guard`
    rows of `fill` on both sides of every head."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(dtype).to(dev)        # noqa: E731
    q, kn, vn = mk(b, HQ, t, D), mk(b, HKV, t, D), mk(b, HKV, t, D)
    kp, vp = mk(b, HQ, P0 + 5, D), mk(b, HQ, P0 + 5, D)
    kfull = torch.full((b, HKV, guard + cap + guard, D), fill, dtype=dtype, device=dev)
    vfull = torch.full_like(kfull, fill)
    kt, vt = kfull[:, :, guard:guard + cap], vfull[:, :, guard:guard + cap]
    live = mk(b, HKV, cap, D), mk(b, HKV, cap, D)
    return q, kn, vn, kp, vp, kt, vt, kfull, vfull, live


def _ws(kvc, q, kn, kp, kt):
    n = kvc.decode_dev_plan(q, kn, kp, P0, kt)[1]
    return torch.empty(max(n, 16), dtype=torch.uint8, device=q.device)


@pytest.mark.parametrize("dtype,D,b,t,T", [(torch.bfloat16, 128, 1, 1, 23), (torch.float32, 64, 3, 3, 87), (torch.bfloat16, 64, 1, 3, 0),
                                           (torch.float32, 128, 3, 1, 215)])
def test_nothing_outside_the_visible_rows_matters(kvc, gpu_device, dtype, D, b, t, T):
    q, kn, vn, kp, vp, kt, vt, _, _, (lk, lv) = _state(gpu_device, dtype, D, b, t, seed=T)
    rows_b = torch.tensor(ROWS3, dtype=torch.int32, device=gpu_device) if b == 3 else None
    counter = torch.tensor([T], dtype=torch.int32, device=gpu_device)
    ws = _ws(kvc, q, kn, kp, kt)
    outs, tails = [], []
    for fill in (float("nan"), 3.0e4):
        kt[:, :, :T], vt[:, :, :T] = lk[:, :, :T], lv[:, :, :T]
        kt[:, :, T:], vt[:, :, T:] = fill, -fill                              # the step's own rows and everything behind them
        kp[:, :, P0:], vp[:, :, P0:] = fill, fill
        ws.view(torch.float32)[:] = fill
        before = (_bits(kt[:, :, T + t:]).clone(), _bits(vt[:, :, T + t:]).clone())
        outs.append(kvc.decode_step_dev(q, kn, vn, kp, vp, P0, kt, vt, counter, D ** -0.5, rows_b=rows_b, ws=ws).clone())
        assert torch.equal(_bits(kt[:, :, T + t:]), before[0]) and torch.equal(_bits(vt[:, :, T + t:]), before[1])
        assert torch.equal(_bits(kt[:, :, T:T + t]), _bits(kn)) and torch.equal(_bits(vt[:, :, T:T + t]), _bits(vn))
        assert torch.equal(_bits(kt[:, :, :T]), _bits(lk[:, :, :T])) and torch.equal(_bits(vt[:, :, :T]), _bits(lv[:, :, :T]))
        tails.append(_bits(kt[:, :, :T + t]).clone())
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(tails[0], tails[1])


@pytest.mark.parametrize("dtype,D,b,t", [(torch.bfloat16, 128, 1, 1), (torch.float32, 64, 3, 3)])
def test_counter_is_clamped_to_the_tail_buffer(kvc, gpu_device, dtype, D, b, t):
    """Counter values -5 and capacity + 100 with the tail a view between 100 + t + 28 guard rows of a sentinel on both sides: the
    guards keep every bit, the output equals the call with the clamped value."""
    guard, sentinel = 100 + t + 28, 12345.0
    rows_b = torch.tensor(ROWS3, dtype=torch.int32, device=gpu_device) if b == 3 else None
    for wild, clamped in ((-5, 0), (CAP + 100, CAP - t)):
        res = []
        for value in (wild, clamped):
            q, kn, vn, kp, vp, kt, vt, kfull, vfull, (lk, lv) = _state(gpu_device, dtype, D, b, t, seed=7, guard=guard, fill=sentinel)
            kt.copy_(lk)
            vt.copy_(lv)
            counter = torch.tensor([value], dtype=torch.int32, device=gpu_device)
            out = kvc.decode_step_dev(q, kn, vn, kp, vp, P0, kt, vt, counter, D ** -0.5, rows_b=rows_b, ws=_ws(kvc, q, kn, kp, kt))
            for full in (kfull, vfull):
                assert (full[:, :, :guard] == sentinel).all() and (full[:, :, guard + CAP:] == sentinel).all(), (wild, value)
            assert int(counter) == value
            res.append((out.clone(), kt.clone(), vt.clone()))
        for x, y in zip(*res):
            assert torch.equal(_bits(x), _bits(y)), wild
        assert torch.equal(_bits(res[0][1][:, :, clamped:clamped + t]), _bits(kn))


def test_captured_call_replays_across_split_boundaries(kvc, gpu_device):
    """One call and the in-graph counter add_ captured on a side stream; 70 replays from T = 20 in the capacity-216 setup (visible rows
    61 .. 130: two boundaries of the 64-row plan) with fresh q / k / v copied into static buffers.  Every replay's out equals an eager
    call of the same entry on a copy of the state; the tails end byte-identical.  Replays run under sync debug mode "error"."""
    dtype, D, b, t, T0, steps = torch.bfloat16, 128, 1, 1, 20, 70
    rps = dev_split_plan(b, HQ, t, P0, CAP)[1]
    assert (P0 + T0 + steps) // rps - (P0 + T0 + t) // rps >= 2              # the visible rows cross two boundaries of the plan
    q, kn, vn, kp, vp, kt, vt, _, _, (lk, lv) = _state(gpu_device, dtype, D, b, t, seed=3)
    kt[:, :, :T0], vt[:, :, :T0] = lk[:, :, :T0], lv[:, :, :T0]
    ekt, evt = kt.clone(), vt.clone()                                       # the eager twin's state
    g = torch.Generator().manual_seed(9)
    feed = [[torch.randn(b, h, t, D, generator=g).to(dtype).to(gpu_device) for h in (HQ, HKV, HKV)] for _ in range(steps)]
    counter = torch.tensor([T0], dtype=torch.int32, device=gpu_device)
    ecounter = counter.clone()
    ws, ews = _ws(kvc, q, kn, kp, kt), _ws(kvc, q, kn, kp, kt)
    out = torch.empty(b, t, HQ, D, dtype=dtype, device=gpu_device)
    kvc.decode_step_dev(q, kn, vn, kp, vp, P0, kt, vt, counter, D ** -0.5, ws=ws, out=out)      # warm-up: row T0 is rewritten below
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(gpu_device), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        kvc.decode_step_dev(q, kn, vn, kp, vp, P0, kt, vt, counter, D ** -0.5, ws=ws, out=out)
        counter.add_(t)
    torch.cuda.synchronize()
    got, want = [], []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fq, fk, fv in feed:
            q.copy_(fq)
            kn.copy_(fk)
            vn.copy_(fv)
            graph.replay()
            got.append(out.clone())
            want.append(kvc.decode_step_dev(fq, fk, fv, kp, vp, P0, ekt, evt, ecounter, D ** -0.5, ws=ews))
            ecounter.add_(t)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert int(counter) == int(ecounter) == T0 + steps
    for j, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(_bits(x), _bits(y)), f"replay {j} (T = {T0 + j})"
    assert torch.equal(_bits(kt), _bits(ekt)) and torch.equal(_bits(vt), _bits(evt))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
def _config(kind="llama", **kw):
    from transformers import LlamaConfig, MistralConfig
    cls = LlamaConfig if kind == "llama" else MistralConfig
    return cls(hidden_size=4096, intermediate_size=256, num_hidden_layers=3, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
               vocab_size=256, max_position_embeddings=4096, attn_implementation="sdpa", eos_token_id=None, pad_token_id=0,
               bos_token_id=None, **kw)


class _Model:
    """The other GPU files' tiny model with the forwards of `method` patched in (restored on exit)."""

    def __init__(self, method, cap=64, window=8, kind="llama", **cfg):
        self.method, self.cap, self.window, self.kind, self.cfg = method, cap, window, kind, cfg

    def __enter__(self):
        from transformers import LlamaForCausalLM, MistralForCausalLM
        from kvcache_factory_amd import monkeypatch as mp
        (mp.replace_llama if self.kind == "llama" else mp.replace_mistral)(self.method)
        torch.manual_seed(0)
        cls = LlamaForCausalLM if self.kind == "llama" else MistralForCausalLM
        model = cls(_config(self.kind, **self.cfg)).to(torch.bfloat16).to("cuda:0").eval()
        for layer in model.model.layers:
            for name, val in (("window_size", self.window), ("max_capacity_prompt", self.cap), ("kernel_size", 7), ("pooling", "maxpool")):
                setattr(layer.self_attn.config, name, val)
        return model

    def __exit__(self, *exc):
        from kvcache_factory_amd import monkeypatch as mp
        (mp.replace_llama if self.kind == "llama" else mp.replace_mistral)("fullkv")


def _ids(n, dev, seed=5):
    return torch.randint(1, 256, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


def _padded(lens, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids, mask = torch.zeros(len(lens), L, dtype=torch.long), torch.zeros(len(lens), L, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, L - n:] = torch.randint(1, 256, (n,), generator=g)
        mask[b, L - n:] = 1
    return ids.to(dev), mask.to(dev)


def _decode(dec, ids, steps, mask=None, watch=False):
    """Greedy: -> (tokens [b, steps], logits of the prefill and of every step, the memory allocated after every replayed step by
    capacity).  Tokens and logits go into buffers made up front, so that the loop itself allocates nothing that stays."""
    from kvcache_factory_amd.graph_decode import tails_needed
    first = dec.prefill(ids, mask)
    logits = torch.empty(steps + 1, *first.shape, dtype=first.dtype, device=first.device)
    toks = torch.empty(first.shape[0], steps, dtype=torch.long, device=first.device)
    logits[0] = first
    mem = collections.defaultdict(list)
    for j in range(steps):
        toks[:, j] = logits[j][:, -1].argmax(-1)
        replay = watch and dec._graph is not None and tails_needed(dec._capacity, dec._tail, 1) == 0
        if replay:
            torch.cuda.set_sync_debug_mode("error")                          # a replayed step never waits for the device
        try:
            logits[j + 1] = dec.step(toks[:, j:j + 1])
        finally:
            torch.cuda.set_sync_debug_mode(0)
        if replay:
            mem[dec._capacity].append(torch.cuda.memory_allocated())
    return toks, list(logits), mem


def _same_layers(a, b):
    for la, lb in zip(a._cache.layers, b._cache.layers):
        assert la._tail == lb._tail and la.get_seq_length() == lb.get_seq_length()
        assert torch.equal(_bits(la.keys), _bits(lb.keys)) and torch.equal(_bits(la.values), _bits(lb.values))


def test_replay_equals_eager_bit_for_bit_and_agrees_with_todays_path(kvc, gpu_device):
    """SnapKV, cap 64, W 8, a 300-token prompt, tail_rows 32, 150 greedy tokens: tokens, every step's logits and the layers' K / V of
    the replayed decoder are bit-identical to capture=False; memory is flat between grow events and no replay synchronises; and
    against today's path (the eager model step over kvc_decode_step2, teacher-forced with the same tokens) every step's logits are
    within 3 % of the largest logit (the bound of test_decode_logits_vs_oracle_built_cache: the split plans differ)."""
    from transformers import DynamicCache
    from kvcache_factory_amd import GraphDecoder
    ids, steps = _ids(300, gpu_device), 150
    with _Model("snapkv") as model:
        a, b = GraphDecoder(model, tail_rows=32), GraphDecoder(model, tail_rows=32, capture=False)
        ta, la, mem = _decode(a, ids, steps, watch=True)
        tb, lb, _ = _decode(b, ids, steps)
        torch.cuda.synchronize()
        assert a.grows >= 2 and a.captures == a.grows + 1 and b.captures == 0 and a.grows == b.grows
        assert torch.equal(ta, tb)
        for j, (x, y) in enumerate(zip(la, lb)):
            assert torch.equal(_bits(x), _bits(y)), f"step {j}"
        _same_layers(a, b)
        assert a._cache.layers[0]._tail == steps and int(a._counter) == steps and a._cache.get_seq_length() == 300 + steps
        assert len(mem) >= 2 and sum(len(v) for v in mem.values()) >= steps - 3 * a.captures
        for cap, seen in mem.items():
            assert len(set(seen)) == 1, f"memory moved between replays at capacity {cap}: {sorted(set(seen))}"
        cache = DynamicCache()
        with torch.no_grad():
            ref = [model(ids, past_key_values=cache, use_cache=True).logits[:, -1:]]
            for j in range(steps):
                ref.append(model(ta[:, j:j + 1], past_key_values=cache, use_cache=True).logits)
        worst = 0.0
        for j, (x, y) in enumerate(zip(la, ref)):
            err, scale = float((x.float() - y.float()).abs().max()), float(y.float().abs().max())
            worst = max(worst, err / scale)
            assert err <= 3e-2 * scale, (j, err, scale)
        print(f"replayed vs host-counted path: worst |logit diff| / max |logit| = {worst:.4f} over {steps + 1} steps")
        assert all(layer._split and not layer._devlen for layer in cache.layers)        # today's path was today's


def test_pyramidkv_layers_of_different_prefix_lengths(kvc, gpu_device):
    from kvcache_factory_amd import GraphDecoder
    ids = _ids(300, gpu_device, seed=6)
    with _Model("pyramidkv") as model:
        a, b = GraphDecoder(model, tail_rows=8), GraphDecoder(model, tail_rows=8, capture=False)
        ta, la, _ = _decode(a, ids, 20)
        tb, lb, _ = _decode(b, ids, 20)
        torch.cuda.synchronize()
        assert len({layer._stored for layer in a._cache.layers}) > 1          # the pyramid: every layer its own budget
        assert torch.equal(ta, tb) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(la, lb))
        _same_layers(a, b)


def test_left_padded_batch(kvc, gpu_device):
    """Three prompts of 300, 100 and 40 tokens (the last below the cap: passed through): replay == eager bit for bit, and every row's
    tokens are those of that prompt decoded alone through GraphDecoder(capture=False)."""
    from kvcache_factory_amd import GraphDecoder
    lens, steps = (300, 100, 40), 12
    ids, mask = _padded(lens, gpu_device)
    with _Model("snapkv") as model:
        a, b = GraphDecoder(model, tail_rows=8), GraphDecoder(model, tail_rows=8, capture=False)
        ta, la, _ = _decode(a, ids, steps, mask)
        tb, lb, _ = _decode(b, ids, steps, mask)
        torch.cuda.synchronize()
        assert a._cache.layers[0].has_holes() and a._cache.layers[0].row_lengths().tolist() == [64, 64, 40]
        assert a._pos.flatten().tolist() == [n + steps for n in lens]
        assert torch.equal(ta, tb) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(la, lb))
        _same_layers(a, b)
        for r, n in enumerate(lens):
            solo, _, _ = _decode(GraphDecoder(model, tail_rows=8, capture=False), ids[r:r + 1, ids.shape[1] - n:], steps)
            assert torch.equal(solo[0], ta[r]), f"row {r}: {solo[0].tolist()} alone, {ta[r].tolist()} in the batch"


def test_generate_is_the_greedy_loop(kvc, gpu_device):
    from kvcache_factory_amd import GraphDecoder
    ids = _ids(120, gpu_device, seed=8)
    with _Model("streamingllm") as model:
        dec = GraphDecoder(model, tail_rows=4)
        out = dec.generate(ids, max_new_tokens=10)
        toks, _, _ = _decode(GraphDecoder(model, tail_rows=4, capture=False), ids, 9)
        torch.cuda.synchronize()
        assert out.shape == (1, 130) and torch.equal(out[:, :120], ids) and torch.equal(out[:, 120:129], toks)
        assert dec.grows == 2 and dec.captures == 3


def test_mistral_without_a_window_works_and_with_one_is_refused(kvc, gpu_device):
    from kvcache_factory_amd import GraphDecoder
    ids = _ids(200, gpu_device, seed=7)
    with _Model("snapkv", kind="mistral", sliding_window=None) as model:
        ta, la, _ = _decode(GraphDecoder(model, tail_rows=4), ids, 10)
        tb, lb, _ = _decode(GraphDecoder(model, tail_rows=4, capture=False), ids, 10)
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(la, lb))
    with _Model("snapkv", kind="mistral", sliding_window=128) as model:
        with pytest.raises(NotImplementedError, match="sliding"):
            GraphDecoder(model)


def test_refusals_raise_before_anything_is_stored(kvc, gpu_device, monkeypatch):
    from transformers import LlamaForCausalLM
    from kvcache_factory_amd import DecodeCompressedCache, GraphDecoder, HeavyHitterCache, KVQuantCompressedCache, QuantizedCompressedCache
    from kvcache_factory_amd import pyramidkv_utils as pu
    ids = _ids(100, gpu_device)
    with pytest.raises(NotImplementedError, match="unpatched"):
        GraphDecoder(LlamaForCausalLM(_config()).to(torch.bfloat16).to(gpu_device).eval())
    for method in ("adakv", "headkv", "think"):
        with _Model(method) as model:
            with pytest.raises(NotImplementedError, match=method):
                GraphDecoder(model)
    with _Model("snapkv") as model:
        cfg = model.config
        for cache, name in ((QuantizedCompressedCache(cfg, nbits=4), "quantized"), (KVQuantCompressedCache(cfg, nbits=4), "quantized"),
                            (DecodeCompressedCache(cfg, interval=8), "DecodeCompressedCache"), (HeavyHitterCache(cfg, interval=8), "HeavyHitterCache")):
            dec = GraphDecoder(model, tail_rows=4)
            with pytest.raises(NotImplementedError, match=name):
                dec.prefill(ids, past_key_values=cache)
            assert dec._cache is None and dec._graph is None and all(layer.get_seq_length() == 0 for layer in cache.layers)
        dec = GraphDecoder(model, tail_rows=4)
        with pytest.raises(NotImplementedError, match="GPU only"):
            dec.prefill(ids.cpu())
        monkeypatch.setattr(pu, "DECODE_KERNEL", False)
        with pytest.raises(NotImplementedError, match="KVC_DECODE_KERNEL=0"):
            dec.prefill(ids)
        monkeypatch.setattr(pu, "DECODE_KERNEL", True)
        monkeypatch.setattr(pu, "BATCH_DECODE", False)
        with pytest.raises(NotImplementedError, match="KVC_BATCH_DECODE=0"):
            dec.prefill(torch.cat([ids, ids]))
        assert dec._cache is None and dec._graph is None and dec.captures == 0
        model.train()
        with pytest.raises(NotImplementedError, match="eval"):
            GraphDecoder(model)
