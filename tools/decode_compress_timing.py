"""Decode-stage compression timing (DecodeCompressedCache / kvc_decode_compress) on one layer of Llama-3-8B geometry: 32 query
heads over 8 KV heads, D 128, bf16, bsz 1, SnapKV, budget B = 2048, interval 128, W in {32, 8}, kernel 7, maxpool, tie mode
torch_cpu.  HIP events; the variants of a measurement alternate in rounds in one process and the median round is reported.
  recompress : one re-compression of S = B + interval rows (P = 2048 prefix rows per query head, T = 128 tail rows per KV head) —
               kvc_decode_compress against materialising cat(prefix, repeat_kv(tail)) + kvc_compress on the same data;
  interval   : us per generated token over a full interval of single-token steps — decode_attend + after_decode (ring writes +
               one re-compression) against the plain fused step over the same stored lengths (P = 2048, T = 0 .. 127);
  long       : step time and cache bytes of the layer after 1k / 4k / 8k generated tokens, without the feature (P = 2048 + a
               T-row tail) and with it (the steady state: the average step over an interval, the bytes the layer holds).
Prints one JSON object per measurement.  --quick: fewer repetitions (for a kernel trace run under rocprofv3)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kvcache_factory_amd import _kvc, pyramidkv_utils as pu
from kvcache_factory_amd.cache import CompressedDynamicLayer, DecodeCompressedLayer

dev = torch.device("cuda:0")
HQ, HKV, D, B, INTERVAL = 32, 8, 128, 2048, 128
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


def recompress(W, g):
    P, T, k = B, INTERVAL, B - W
    kp, vp, kt, vt, ring = rnd(g, 1, HQ, P + 256, D), rnd(g, 1, HQ, P + 256, D), rnd(g, 1, HKV, 256, D), rnd(g, 1, HKV, 256, D), rnd(g, 1, HQ, W, D)
    kb, vb = torch.empty(1, HQ, B, D, dtype=dt, device=dev), torch.empty(1, HQ, B, D, dtype=dt, device=dev)
    qfull = torch.zeros(1, HQ, P + T, D, dtype=dt, device=dev)
    qfull[:, :, P + T - W:] = ring

    def new():
        _kvc.decode_compress(_kvc.SNAPKV, ring, 0, kp, vp, P, kt, vt, T, (kb, vb), W, k, 7, "maxpool", pu.TIE_MODE)

    def materialised():
        K = torch.cat([kp[:, :, :P], kt[:, :, :T].repeat_interleave(HQ // HKV, 1)], 2)
        V = torch.cat([vp[:, :, :P], vt[:, :, :T].repeat_interleave(HQ // HKV, 1)], 2)
        _kvc.compress(_kvc.SNAPKV, qfull, K, V, W, k, 7, "maxpool", pu.TIE_MODE, dot_mode="exact", out=(kb, vb))

    t_new, t_mat = median_rounds([new, materialised], 5 if QUICK else 20, 3 if QUICK else 9)
    es = 2
    scan = (P * HQ + T * HKV) * D * es                       # K read once by the window scan
    gather = 2 * 2 * B * HQ * D * es                         # K and V rows read and written
    mat = 2 * 2 * (P + T) * HQ * D * es                      # cat: K and V written, then read again by kvc_compress's scan / gather
    return dict(measure="recompress", W=W, S=P + T, us_decode_compress=round(t_new, 1), us_materialise_compress=round(t_mat, 1),
                speedup=round(t_mat / t_new, 2), mb_scan=round(scan / 1e6, 1), mb_gather=round(gather / 1e6, 1),
                mb_materialise_extra=round(mat / 1e6, 1))


def prefilled(cls, g, P, *args):
    layer = cls(*args)
    layer.prefill(rnd(g, 1, HQ, P, D), rnd(g, 1, HQ, P, D), 100000)
    return layer


def interval_cost(W, g):
    cl = pu.SnapKVCluster(window_size=W, max_capacity_prompt=B, kernel_size=7, pooling="maxpool")
    steps = [(rnd(g, 1, HQ, 1, D), rnd(g, 1, HKV, 1, D), rnd(g, 1, HKV, 1, D)) for _ in range(INTERVAL)]
    on = prefilled(DecodeCompressedLayer, g, B, INTERVAL)
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

    run_on()                                                 # first interval: allocations, first compression
    n0 = on.compressions
    t_on, t_off = median_rounds([run_on, run_off], 1 if QUICK else 3, 3 if QUICK else 9)
    assert on.compressions > n0 and on.rows()[1] == 0
    return dict(measure="interval", W=W, us_per_token_on=round(t_on / INTERVAL, 2), us_per_token_plain=round(t_off / INTERVAL, 2),
                overhead_pct=round(100 * (t_on / t_off - 1), 1))


def long_generation(g):
    W = 32
    cl = pu.SnapKVCluster(window_size=W, max_capacity_prompt=B, kernel_size=7, pooling="maxpool")
    q, k, v = rnd(g, 1, HQ, 1, D), rnd(g, 1, HKV, 1, D), rnd(g, 1, HKV, 1, D)
    sc = D ** -0.5
    out = []
    on = prefilled(DecodeCompressedLayer, g, B, INTERVAL)
    steps = [(rnd(g, 1, HQ, 1, D), rnd(g, 1, HKV, 1, D), rnd(g, 1, HKV, 1, D)) for _ in range(INTERVAL)]

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
    res = []
    for W in (32, 8):
        res.append(recompress(W, g))
        print(json.dumps(res[-1]), flush=True)
    for W in (32, 8):
        res.append(interval_cost(W, g))
        print(json.dumps(res[-1]), flush=True)
    for r in long_generation(g):
        res.append(r)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
