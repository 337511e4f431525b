"""us per decode step per layer of the quantized cache (kvc_decode_step_quant at 2 / 4 / 8 bits) beside the bf16 step
(kvc_decode_step2) on the same cache contents, Llama-3-8B head geometry (32 query heads over 8 KV heads, D 128, bsz 1, one new
token), prefix P in {136, 2056} rows per query head, T in {0, 1024} decoded rows per KV head (quantized: T - 32 rows on the
quantized tail in whole groups of G = 64, 32 in the full-precision residual; R = 128).  Device events over `reps` calls, after a
warm-up, the bf16 and the quantized step alternating in rounds in the same process; the median round is reported.
Bytes a step must read per query head (the prefix, the KV head's tail / residual, metadata), over the kernel-time estimate of the
median, against the 8 TB/s HBM peak.  Prints one JSON object per configuration and a summary."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kvcache_factory_amd import _kvc

dev = torch.device("cuda:0")
HQ, HKV, D, G, R, RES = 32, 8, 128, 64, 128, 32
dt = torch.bfloat16
scaling = D ** -0.5
HBM = 8.0e12


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


def main():
    g = torch.Generator().manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dt).to(dev)        # noqa: E731
    results = []
    for P in (136, 2056):
        for T in (0, 1024):
            q, kn, vn = rn(1, HQ, 1, D), rn(1, HKV, 1, D), rn(1, HKV, 1, D)
            kp, vp = rn(1, HQ, P + 256, D), rn(1, HQ, P + 256, D)
            kt, vt = rn(1, HKV, T + 64, D), rn(1, HKV, T + 64, D)
            bf16 = lambda: _kvc.decode_step(q, kn, vn, kp, vp, P, kt, vt, T, scaling)             # noqa: E731
            fns, names, nbytes = [bf16], ["bf16"], [(P + T) * D * 2 * 2]
            tq = max(T - RES, 0) // G * G
            res = T - tq
            for nbits in (2, 4, 8):
                pre = _kvc.quant_buffers(1, HQ, P, D, nbits, G, dev)
                _kvc.quantize_rows(kp[:, :, :P], pre[0], pre[2], 0, _kvc.QUANT_KEYS, nbits, G)
                _kvc.quantize_rows(vp[:, :, :P], pre[1], pre[3], 0, _kvc.QUANT_VALUES, nbits, G)
                tail = None
                if tq:
                    tb = _kvc.quant_buffers(1, HKV, tq, D, nbits, G, dev)
                    _kvc.quantize_rows(kt[:, :, :tq], tb[0], tb[2], 0, _kvc.QUANT_KEYS, nbits, G)
                    _kvc.quantize_rows(vt[:, :, :tq], tb[1], tb[3], 0, _kvc.QUANT_VALUES, nbits, G)
                    tail = (*tb, tq)
                kr, vr = rn(1, HKV, R + 64, D), rn(1, HKV, R + 64, D)
                kr[:, :, :res].copy_(kt[:, :, tq:T])
                vr[:, :, :res].copy_(vt[:, :, tq:T])
                seg = (*pre, P)
                fns.append(lambda seg=seg, tail=tail, kr=kr, vr=vr, nb=nbits:
                           _kvc.decode_step_quant(q, kn, vn, seg, tail, kr, vr, res, scaling, nb, G, R))
                names.append(f"q{nbits}")
                rows_q = P + tq
                nbytes.append(rows_q * (D * nbits // 8 * 2 + D // G * 8) + -(-P // G) * 2 * D * 4 + (tq // G) * 2 * D * 4
                              + (res + 1) * D * 2 * 2)
            ref = bf16().float()
            errs = [float((f().float() - ref).abs().max()) for f in fns[1:]]
            for f in fns:                                                 # warm-up of every shape
                for _ in range(20):
                    f()
            torch.cuda.synchronize()
            rounds = [time_round(fns, 100) for _ in range(7)]
            med = [statistics.median(r[i] for r in rounds) for i in range(len(fns))]
            row = {"prefix_rows": P, "tail_rows": T, "quant_tail_rows": tq, "residual_rows": res}
            for i, n in enumerate(names):
                row[f"{n}_us"] = round(med[i], 2)
                row[f"{n}_bytes_per_head"] = nbytes[i]
                row[f"{n}_hbm_frac"] = round(nbytes[i] * HQ / (med[i] * 1e-6) / HBM, 4)
                if i:
                    row[f"{n}_vs_bf16"] = round(med[0] / med[i], 3)
                    row[f"{n}_max_abs_diff_vs_bf16"] = errs[i - 1]
            print(json.dumps(row), flush=True)
            results.append(row)
    print(json.dumps({"geometry": "H_q 32, H_kv 8, D 128, bf16, bsz 1, one new token, G 64, R 128", "unit": "us per step per layer",
                      "timing": "HIP events, 7 alternating rounds of 100 calls, median", "results": results}))


if __name__ == "__main__":
    main()
