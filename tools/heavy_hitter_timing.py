"""Heavy-hitter cache timing (HeavyHitterCache / kvc_decode_step_scored / kvc_decode_evict) on one layer of Llama-3-8B geometry:
32 query heads over 8 KV heads, D 128, bf16, bsz 1, budget B = 2048, interval 128, W = 32.  HIP events; the variants of a
measurement alternate in rounds in one process and the median round is reported.
  step     : us per step at P = 2048, T = 64 of (a) kvc_decode_step_scored, (b) kvc_decode_step2 at the same lengths, (c) the
             way to the same scores without it: repeat_kv + append + eager attention that returns its weights + the column add.
             Gate: (a) <= (c).  (a) against (b) is the price of scoring.
  evict    : one eviction at S = 2176 beside kvc_decode_compress (SnapKV maxpool 7, W = 32) on the same shape, both tie modes;
  interval : us per generated token over a full interval of single-token steps, HeavyHitterLayer against the plain fused step
             over the same stored lengths;
  long     : step time and bytes of the layer after 1k / 4k / 8k generated tokens against the plain growing cache.
Prints one JSON object per measurement.  --quick: fewer repetitions (for a kernel trace run under rocprofv3)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kvcache_factory_amd import _kvc, pyramidkv_utils as pu
from kvcache_factory_amd.cache import CompressedDynamicLayer, HeavyHitterLayer

dev = torch.device("cuda:0")
HQ, HKV, D, B, INTERVAL, W = 32, 8, 128, 2048, 128, 32
dt = torch.bfloat16
QUICK = "--quick" in sys.argv


def rnd(g, *shape):
    return torch.randn(*shape, generator=g).to(dt).to(dev)


def events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def median_rounds(fns, reps, rounds):
    for f in fns:
        f()
    torch.cuda.synchronize()
    rr = [[events_us(f, reps) for f in fns] for _ in range(rounds)]
    return [statistics.median(r[i] for r in rr) for i in range(len(fns))]


def layer_bytes(layer):
    return sum(getattr(layer, n).numel() * getattr(layer, n).element_size() for n in layer._batch_tensors
               if getattr(layer, n) is not None)


def step(g):
    P, T, G, sc = B, 64, HQ // HKV, D ** -0.5
    kp, vp, kt, vt = rnd(g, 1, HQ, P, D), rnd(g, 1, HQ, P, D), rnd(g, 1, HKV, 256, D), rnd(g, 1, HKV, 256, D)
    sp = torch.zeros(1, HQ, P, dtype=torch.float32, device=dev)
    st = torch.zeros(1, HQ, 256, dtype=torch.float32, device=dev)
    q, k, v = rnd(g, 1, HQ, 1, D), rnd(g, 1, HKV, 1, D), rnd(g, 1, HKV, 1, D)
    Ke = torch.cat([kp, kt[:, :, :T].repeat_interleave(G, 1)], 2).contiguous()        # the reference-shaped cache [1, H_q, S, D]
    Ve = torch.cat([vp, vt[:, :, :T].repeat_interleave(G, 1)], 2).contiguous()
    acc = torch.zeros(1, HQ, P + T + 1, dtype=torch.float32, device=dev)

    def scored():
        _kvc.decode_step_scored(q, k, v, kp, vp, P, kt, vt, T, sp, st, sc)

    def plain():
        _kvc.decode_step(q, k, v, kp, vp, P, kt, vt, T, sc)

    def eager():                                   # output_attentions=True: repeat_kv + cat + eager softmax with the weights kept
        K = torch.cat([Ke, k.repeat_interleave(G, 1)], 2)
        V = torch.cat([Ve, v.repeat_interleave(G, 1)], 2)
        w = torch.softmax((q @ K.transpose(2, 3)) * sc, dim=-1, dtype=torch.float32)
        out = (w.to(dt) @ V).transpose(1, 2).contiguous()
        acc.add_(w[:, :, 0])
        return out

    a, b, c = median_rounds([scored, plain, eager], 20 if QUICK else 200, 3 if QUICK else 9)
    rows = P + T + 1
    return dict(measure="step", P=P, T=T, us_scored=round(a, 2), us_step2=round(b, 2), us_eager_weights=round(c, 2),
                scoring_price_us=round(a - b, 2), gate_scored_le_eager=bool(a <= c),
                mb_kv_read=round(2 * (P * HQ + (T + 1) * HKV) * D * 2 / 1e6, 1), mb_logits_written_and_read=round(2 * HQ * rows * 4 / 1e6, 2),
                mb_scores_read_and_written=round(2 * HQ * rows * 4 / 1e6, 2))


def evict(g):
    P, T, k = B, INTERVAL, B - W
    kp, vp, kt, vt, ring = rnd(g, 1, HQ, P, D), rnd(g, 1, HQ, P, D), rnd(g, 1, HKV, 256, D), rnd(g, 1, HKV, 256, D), rnd(g, 1, HQ, W, D)
    sp = (torch.rand(1, HQ, P, generator=g) * 10).to(dev)
    st = (torch.rand(1, HQ, 256, generator=g)).to(dev)
    kb, vb = torch.empty(1, HQ, B, D, dtype=dt, device=dev), torch.empty(1, HQ, B, D, dtype=dt, device=dev)
    sb = torch.empty(1, HQ, B, dtype=torch.float32, device=dev)
    out = []
    for tie in ("torch_cpu", "canonical"):
        def ev():
            _kvc.decode_evict(kp, vp, P, kt, vt, T, sp, st, (kb, vb), sb, W, k, tie)

        def dc():
            _kvc.decode_compress(_kvc.SNAPKV, ring, 0, kp, vp, P, kt, vt, T, (kb, vb), W, k, 7, "maxpool", tie)

        t_ev, t_dc = median_rounds([ev, dc], 5 if QUICK else 20, 3 if QUICK else 9)
        out.append(dict(measure="evict", tie_mode=tie, S=P + T, us_decode_evict=round(t_ev, 1), us_decode_compress=round(t_dc, 1)))
    return out


def prefilled(cls, g, P, *args):
    layer = cls(*args)
    layer.prefill(rnd(g, 1, HQ, P, D), rnd(g, 1, HQ, P, D), 100000)
    return layer


def make_steps(g):
    return [(rnd(g, 1, HQ, 1, D), rnd(g, 1, HKV, 1, D), rnd(g, 1, HKV, 1, D)) for _ in range(INTERVAL)]


def interval_cost(g):
    cl = pu.H2OKVCluster(window_size=W, max_capacity_prompt=B)
    steps = make_steps(g)
    on = prefilled(HeavyHitterLayer, g, B, INTERVAL)
    off = prefilled(CompressedDynamicLayer, g, B)
    sc = D ** -0.5

    def run_on():
        for q, k, v in steps:
            on.decode_attend(q, k, v, sc)
            on.after_decode(cl, q)

    def run_off():
        for q, k, v in steps:
            off.decode_attend(q, k, v, sc)
        off._tail = 0                                        # the same stored lengths every interval

    run_on()                                                 # first interval: allocations, first eviction
    n0 = on.evictions
    t_on, t_off = median_rounds([run_on, run_off], 1 if QUICK else 3, 3 if QUICK else 9)
    assert on.evictions > n0 and on.rows()[1] == 0
    return dict(measure="interval", tie_mode=pu.TIE_MODE, us_per_token_on=round(t_on / INTERVAL, 2),
                us_per_token_plain=round(t_off / INTERVAL, 2), overhead_pct=round(100 * (t_on / t_off - 1), 1))


def long_generation(g):
    cl = pu.H2OKVCluster(window_size=W, max_capacity_prompt=B)
    q, k, v = rnd(g, 1, HQ, 1, D), rnd(g, 1, HKV, 1, D), rnd(g, 1, HKV, 1, D)
    sc = D ** -0.5
    out = []
    on = prefilled(HeavyHitterLayer, g, B, INTERVAL)
    steps = make_steps(g)

    def run_on():
        for qq, kk, vv in steps:
            on.decode_attend(qq, kk, vv, sc)
            on.after_decode(cl, qq)
    for n in (1024, 4096, 8192):
        off = prefilled(CompressedDynamicLayer, g, B)
        off.decode_attend(q, k, v, sc)
        t = n - 1
        kt = torch.empty(1, HKV, n + 256, D, dtype=dt, device=dev)
        kt[:, :, :t] = rnd(g, 1, HKV, t, D)
        off._ktail, off._vtail, off._tail = kt, kt.clone(), t      # the plain layer after n generated tokens

        def step_off():
            off.decode_attend(q, k, v, sc)
            off._tail = t
        while on.true_length < 100000 + n:                           # the feature's layer after n generated tokens
            run_on()
        t_off, t_on = median_rounds([step_off, run_on], 5 if QUICK else 20, 3 if QUICK else 7)
        out.append(dict(measure="long", tokens=n, us_step_plain=round(t_off, 1), us_step_on=round(t_on / INTERVAL, 1),
                        mb_plain=round(layer_bytes(off) / 1e6, 1), mb_on=round(layer_bytes(on) / 1e6, 1)))
    return out


def main():
    g = torch.Generator().manual_seed(0)
    print(json.dumps(step(g)), flush=True)
    for r in evict(g):
        print(json.dumps(r), flush=True)
    print(json.dumps(interval_cost(g)), flush=True)
    for r in long_generation(g):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
