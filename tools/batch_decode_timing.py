"""us per decode step per layer for a BATCH (bsz 8, Llama-3-8B head geometry: 32 query heads over 8 KV heads, D 128, bf16, one
new token, tail 256), uniform prefix rows [2056] * 8 and unequal ones [2056, 2056, 1032, 520, 264, 136, 72, 40]:
  (a) one kvc_decode_step_rows call;
  (b) the same work as eight bsz = 1 kvc_decode_step2 calls on the row slices (what per-prompt decoding costs);
  (c) the reference-shaped batch path: repeat_kv of the new token, append, SDPA with a mask over [8, 32, rows_max + tail + 1, 128].
The three are timed in ONE process, alternating (a, b, c, a, b, c, ...) after a warm-up, each step between two device events;
medians over `STEPS` steps, and the spread of (b)'s medians over `RUNS` repeated runs.  Prints one JSON object."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from kvcache_factory_amd import _kvc
dev = torch.device("cuda:0")
B, HQ, HKV, D, G, T = 8, 32, 8, 128, 4, 256
dt = torch.bfloat16
scaling = D ** -0.5
STEPS, WARM, RUNS = 200, 20, 3
SETS = {"uniform": [2056] * 8, "unequal": [2056, 2056, 1032, 520, 264, 136, 72, 40]}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


out = {"geometry": "bsz 8, H_q 32, H_kv 8, D 128, bf16, one new token, tail 256", "unit": "us per step per layer (median of %d)" % STEPS,
       "sets": {}}
g = torch.Generator(device="cpu").manual_seed(0)
rn = lambda *sh: torch.randn(*sh, generator=g).to(dt).to(dev)      # noqa: E731
for name, rows in SETS.items():
    pmax = max(rows)
    kp, vp = rn(B, HQ, pmax + 256, D), rn(B, HQ, pmax + 256, D)
    kt, vt = rn(B, HKV, T + 64, D), rn(B, HKV, T + 64, D)
    q, kn, vn = rn(B, HQ, 1, D), rn(B, HKV, 1, D), rn(B, HKV, 1, D)
    rows_b = torch.tensor(rows, dtype=torch.int32, device=dev)
    # (c): the reference-shaped cache [8, 32, rows_max + T + 1, 128] with the layer's additive mask over the holes
    kc = torch.cat([kp[:, :, :pmax], kt[:, :, :T].repeat_interleave(G, 1), kp[:, :, :1]], 2).contiguous()
    vc = torch.cat([vp[:, :, :pmax], vt[:, :, :T].repeat_interleave(G, 1), vp[:, :, :1]], 2).contiguous()
    col = torch.arange(pmax + T + 1, device=dev)
    hole = (col[None, :] >= rows_b[:, None]) & (col[None, :] < pmax)
    mask = torch.zeros(B, 1, 1, pmax + T + 1, dtype=dt, device=dev).masked_fill(hole[:, None, None, :], float("-inf"))
    slices = [(q[r:r + 1], kn[r:r + 1], vn[r:r + 1], kp[r:r + 1], vp[r:r + 1], kt[r:r + 1], vt[r:r + 1]) for r in range(B)]

    def rows_call():
        return _kvc.decode_step_rows(q, kn, vn, kp, vp, rows_b, pmax, kt, vt, T, scaling)

    def eight_calls():
        return [_kvc.decode_step(s[0], s[1], s[2], s[3], s[4], rows[r], s[5], s[6], T, scaling) for r, s in enumerate(slices)]

    def ref_shaped():
        kc[:, :, pmax + T:] = kn[:, :, None].expand(B, HKV, G, 1, D).reshape(B, HQ, 1, D)
        vc[:, :, pmax + T:] = vn[:, :, None].expand(B, HKV, G, 1, D).reshape(B, HQ, 1, D)
        return F.scaled_dot_product_attention(q, kc, vc, attn_mask=mask)
    oa, ob, oc = rows_call(), torch.cat(eight_calls(), 0), ref_shaped().transpose(1, 2)
    res = {"prefix_rows": rows, "total_rows": sum(rows) + B * T, "max_abs_diff_a_vs_b": float((oa.float() - ob.float()).abs().max()),
           "max_abs_diff_a_vs_c": float((oa.float() - oc.float()).abs().max()), "runs": []}
    fns = (("a_decode_step_rows", rows_call), ("b_eight_decode_step2", eight_calls), ("c_repeat_kv_append_sdpa_mask", ref_shaped))
    for run in range(RUNS):
        for _ in range(WARM):
            for _, fn in fns:
                fn()
        evs = {n: [] for n, _ in fns}
        for _ in range(STEPS):
            for n, fn in fns:
                evs[n].append(timed(fn))
        torch.cuda.synchronize()
        res["runs"].append({n: round(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in v), 2) for n, v in evs.items()})
        print(name, res["runs"][-1], flush=True)
    med = {n: statistics.median(r[n] for r in res["runs"]) for n, _ in fns}
    bs = [r["b_eight_decode_step2"] for r in res["runs"]]
    res.update(median_us=med, b_spread_us=round(max(bs) - min(bs), 2),
               a_over_b=round(med["a_decode_step_rows"] / med["b_eight_decode_step2"], 3),
               c_over_a=round(med["c_repeat_kv_append_sdpa_mask"] / med["a_decode_step_rows"], 2))
    out["sets"][name] = res
u, n = out["sets"]["uniform"], out["sets"]["unequal"]
out["unequal_over_uniform"] = {"a_time_ratio": round(n["median_us"]["a_decode_step_rows"] / u["median_us"]["a_decode_step_rows"], 3),
                               "total_rows_ratio": round(n["total_rows"] / u["total_rows"], 3)}
print(json.dumps(out))
