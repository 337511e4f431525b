"""us per decode step per layer of the quantized cache with exact outliers (kvc_decode_step_quant_outliers) beside the KIVI step
(kvc_decode_step_quant) and the bf16 step (kvc_decode_step2) on the same cache contents; geometry and method of
tools/quant_decode_timing.py: 32 query heads over 8 KV heads, D 128, bf16, bsz 1, one new token, P in {136, 2056} prefix rows per
query head, T in {0, 1024} decoded rows per KV head (T - 32 on the quantized tail in groups of G = 64, 32 in the residual; R = 128),
nbits 2 / 4 / 8.  Outlier patterns (T = 6): `none` (no element above T), `random` (1 % of the elements at +-40), `channels` (two
whole key channels spread over +-40).  HIP events over `reps` calls after a warm-up, the three steps alternating in rounds in one
process; the median round is reported.  Also the time of the quantize calls (KIVI and with outliers) for the prompt and for one
flush of R rows.  Prints one JSON object per configuration and a summary."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kvcache_factory_amd import _kvc

dev = torch.device("cuda:0")
HQ, HKV, D, G, R, RES, T = 32, 8, 128, 64, 128, 32, 6.0
dt = torch.bfloat16
scaling = D ** -0.5


def time_round(fns, reps):
    out = []
    for fn in fns:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return out


def median_times(fns, reps=100, rounds=7):
    for f in fns:
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    rr = [time_round(fns, reps) for _ in range(rounds)]
    return [statistics.median(r[i] for r in rr) for i in range(len(fns))]


def data(g, heads, rows, pattern, key):
    x = torch.randn(1, heads, rows, D, generator=g).clamp(-5.5, 5.5)
    if pattern == "random":
        sel = torch.rand(1, heads, rows, D, generator=g) < 0.01
        x[sel] = 40 * torch.sign(torch.randn(int(sel.sum()), generator=g))
    elif pattern == "channels" and key:
        x[:, :, :, [17, 90]] = (torch.rand(1, heads, rows, 2, generator=g) * 2 - 1) * 40
    return x.to(dt).to(dev)


def quantize_both(k, v, heads, rows, nbits, outl):
    bufs = _kvc.quant_buffers(1, heads, rows, D, nbits, G, dev)
    if not outl:
        _kvc.quantize_rows(k, bufs[0], bufs[2], 0, _kvc.QUANT_KEYS, nbits, G)
        _kvc.quantize_rows(v, bufs[1], bufs[3], 0, _kvc.QUANT_VALUES, nbits, G)
        return bufs, None
    pools = [_kvc.outlier_pool(1, heads, rows, max(16, heads * rows * D // 8), dt, dev) for _ in range(2)]
    _kvc.quantize_rows_outliers(k, bufs[0], bufs[2], pools[0], 0, _kvc.QUANT_KEYS, nbits, G, T)
    _kvc.quantize_rows_outliers(v, bufs[1], bufs[3], pools[1], 0, _kvc.QUANT_VALUES, nbits, G, T)
    return bufs, pools


def main():
    g = torch.Generator().manual_seed(0)
    results, qtimes = [], []
    for P in (136, 2056):
        for Tr in (0, 1024):
            for pattern in ("none", "random", "channels"):
                q = torch.randn(1, HQ, 1, D, generator=g).to(dt).to(dev)
                kn, vn = data(g, HKV, 1, "none", True), data(g, HKV, 1, "none", False)
                kp, vp = torch.empty(1, HQ, P + 256, D, dtype=dt, device=dev), torch.empty(1, HQ, P + 256, D, dtype=dt, device=dev)
                kp[:, :, :P], vp[:, :, :P] = data(g, HQ, P, pattern, True), data(g, HQ, P, pattern, False)
                kt, vt = torch.empty(1, HKV, Tr + 64, D, dtype=dt, device=dev), torch.empty(1, HKV, Tr + 64, D, dtype=dt, device=dev)
                kt[:, :, :Tr], vt[:, :, :Tr] = data(g, HKV, Tr, pattern, True), data(g, HKV, Tr, pattern, False)
                fns = [lambda: _kvc.decode_step(q, kn, vn, kp, vp, P, kt, vt, Tr, scaling)]
                names = ["bf16"]
                tq = max(Tr - RES, 0) // G * G
                res = Tr - tq
                for nbits in (2, 4, 8):
                    kr, vr = torch.empty(1, HKV, R + 64, D, dtype=dt, device=dev), torch.empty(1, HKV, R + 64, D, dtype=dt, device=dev)
                    kr[:, :, :res], vr[:, :, :res] = kt[:, :, tq:Tr], vt[:, :, tq:Tr]
                    kq, _ = quantize_both(kp[:, :, :P], vp[:, :, :P], HQ, P, nbits, False)
                    ko, po = quantize_both(kp[:, :, :P], vp[:, :, :P], HQ, P, nbits, True)
                    tk = tko = tpo = None
                    if tq:
                        tk, _ = quantize_both(kt[:, :, :tq], vt[:, :, :tq], HKV, tq, nbits, False)
                        tko, tpo = quantize_both(kt[:, :, :tq], vt[:, :, :tq], HKV, tq, nbits, True)
                    fns.append(lambda kq=kq, tk=tk, kr=kr, vr=vr, nb=nbits: _kvc.decode_step_quant(
                        q, kn, vn, (*kq, P), (*tk, tq) if tk else None, kr, vr, res, scaling, nb, G, R))
                    fns.append(lambda ko=ko, po=po, tko=tko, tpo=tpo, kr=kr, vr=vr, nb=nbits: _kvc.decode_step_quant_outliers(
                        q, kn, vn, (*ko, P), (*tko, tq) if tko else None, po, tpo, kr, vr, res, scaling, nb, G, R))
                    names += [f"kivi{nbits}", f"kvq{nbits}"]
                med = median_times(fns)
                row = {"prefix_rows": P, "tail_rows": Tr, "pattern": pattern, "quant_tail_rows": tq, "residual_rows": res}
                for i, n in enumerate(names):
                    row[f"{n}_us"] = round(med[i], 2)
                for nbits in (2, 4, 8):
                    row[f"kvq{nbits}_vs_kivi"] = round(med[names.index(f"kvq{nbits}")] / med[names.index(f"kivi{nbits}")], 3)
                    row[f"kvq{nbits}_vs_bf16"] = round(med[names.index(f"kvq{nbits}")] / med[0], 3)
                if pattern != "none":
                    row["prefix_outliers_k_v"] = [int(po[0][2][0]), int(po[1][2][0])]
                print(json.dumps(row), flush=True)
                results.append(row)
    # quantize calls: the prompt (P rows per query head) and one flush (R rows per KV head), keys + values, 4 bits
    for what, heads, rows in (("prompt", HQ, 2056), ("prompt", HQ, 136), ("flush", HKV, R)):
        for pattern in ("none", "random"):
            k, v = data(g, heads, rows, pattern, True), data(g, heads, rows, pattern, False)
            bufs = _kvc.quant_buffers(1, heads, rows, D, 4, G, dev)
            pools = [_kvc.outlier_pool(1, heads, rows, heads * rows * D // 4, dt, dev) for _ in range(2)]

            def kivi():
                _kvc.quantize_rows(k, bufs[0], bufs[2], 0, _kvc.QUANT_KEYS, 4, G)
                _kvc.quantize_rows(v, bufs[1], bufs[3], 0, _kvc.QUANT_VALUES, 4, G)

            def kvq():
                for p in pools:
                    p[2].zero_()
                _kvc.quantize_rows_outliers(k, bufs[0], bufs[2], pools[0], 0, _kvc.QUANT_KEYS, 4, G, T)
                _kvc.quantize_rows_outliers(v, bufs[1], bufs[3], pools[1], 0, _kvc.QUANT_VALUES, 4, G, T)

            def zero():
                for p in pools:
                    p[2].zero_()
            med = median_times([kivi, kvq, zero], reps=50)
            row = {"quantize": what, "heads": heads, "rows": rows, "pattern": pattern, "kivi_us": round(med[0], 2),
                   "kvq_us": round(med[1] - med[2], 2)}
            print(json.dumps(row), flush=True)
            qtimes.append(row)
    print(json.dumps({"geometry": "H_q 32, H_kv 8, D 128, bf16, bsz 1, one new token, G 64, R 128, T 6", "unit": "us per step per layer",
                      "timing": "HIP events, 7 alternating rounds of 100 calls, median", "results": results, "quantize": qtimes}))


if __name__ == "__main__":
    main()
