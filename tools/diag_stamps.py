"""Phase breakdown of logits_kernel from the -DKVC_STAMPS diagnostic build (tools/diag/libkvc_hip_stamps.so).
Run with KVC_LIB_PATH pointing at that library.  Shares only — never quote this build's run time.
KVC_STAMPS_LOGITS_ONLY=1 stops after the logits_kernel table."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from kvcache_factory_amd import _kvc, synth
dev = torch.device("cuda:0")
W = int(sys.argv[1]) if len(sys.argv) > 1 else 8
BSZ = int(sys.argv[2]) if len(sys.argv) > 2 else 32           # 32 x 8 KV heads in one call: the benchmark's batch geometry
q, k, v = synth.make_qkv(32, 8, 8000, 128, torch.bfloat16, 0, bsz=BSZ, device=dev)
p = _kvc.make_params(_kvc.SNAPKV, q, k, None, W, 0, 7, "maxpool")
p.debug_stage_mask = 1
nbytes = _kvc.lib().kvc_workspace_bytes(ctypes.byref(p)); ws = _kvc.workspace(dev, nbytes)
sc = torch.zeros(1 << 20, dtype=torch.int64, device=dev)     # stamps land here
st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
for it in range(5):
    sc.zero_()
    rc = _kvc.lib().kvc_scores(ctypes.byref(p), _kvc._ptr(q), _kvc._ptr(k), _kvc._ptr(sc), _kvc._ptr(ws), nbytes, st)
    assert rc == 0, _kvc.lib().kvc_last_error()
    torch.cuda.synchronize()
def groups_per_head(L, units):                                  # kvc_api.hip: carve()
    tiles32, best, best_g = (L + 31) // 32, 1e30, 1
    for g in range(1, (tiles32 + 3) // 4 + 1):
        cost = -(-g * units // 768) * (-(-tiles32 // (4 * g)) + 1.5)
        if cost < best - 1e-9:
            best, best_g = cost, g
    return best_g
nblk = groups_per_head(8000, BSZ * 8) * BSZ * 8
# per wave: slot 0 = first stamp, slot p = ticks of the phase that ENDS at stamp p summed over the wave's tiles, slot 7 = tiles
t = sc[: nblk * 4 * 8].view(nblk * 4, 8).cpu().double()
names = {1: "prologue: Q image, first tile's loads and commit",
         2: "issue next tile's loads (+ any wait before the chain)",
         3: "MFMA chain (+LDS reads), commit of the next tile",
         5: "epilogue: round/div/mask, maxima, stores",
         6: "row-max fold, block maximum"}
tot = t[:, [1, 2, 3, 5, 6]].sum(1)
print("waves", t.shape[0], " tiles per wave: mean %.2f" % float(t[:, 7].mean()), " (s_memtime ticks of the constant clock; shares only)")
for i, nm in names.items():
    per_tile = (t[:, i] / t[:, 7].clamp(min=1)).mean() if i in (2, 3, 5) else float("nan")
    print(f"  {nm:55s} mean {t[:, i].mean():9.1f}  share {100 * t[:, i].sum() / tot.sum():5.1f} %  per tile {per_tile:8.1f}")
print("  wave total mean", float(tot.mean()), " max", float(tot.max()))
s0 = t[:, 0] - t[:, 0].min()
print("  wave start offsets: p50", float(s0.median()), "p90", float(s0.quantile(0.9)), "max", float(s0.max()))
end = t[:, 0] + tot
print("  kernel span", float(end.max() - t[:, 0].min()))
if os.environ.get("KVC_STAMPS_LOGITS_ONLY"):
    sys.exit(0)

# ---- select_kernel phases (wave 0 of each head) ----
del q, k, v
q, k, v = synth.make_qkv(32, 8, 8000, 128, torch.bfloat16, 0, device=dev)
p2 = _kvc.make_params(_kvc.SNAPKV, q, k, v, W, 120, 7, "maxpool", "canonical")
ko = torch.empty(1, 32, 128, 128, dtype=torch.bfloat16, device=dev); vo = torch.empty_like(ko)
idx = torch.zeros(1, 32, 120, dtype=torch.int64, device=dev)
nb = _kvc.lib().kvc_workspace_bytes(ctypes.byref(p2)); ws2 = _kvc.workspace(dev, nb)
for it in range(3):
    rc = _kvc.lib().kvc_compress(ctypes.byref(p2), _kvc._ptr(q), _kvc._ptr(k), _kvc._ptr(v), _kvc._ptr(ko), _kvc._ptr(vo), _kvc._ptr(idx), None, _kvc._ptr(ws2), nb, st)
    assert rc == 0, _kvc.lib().kvc_last_error()
    torch.cuda.synchronize()
ts = idx[0, :, :6].cpu().double()
dd = ts[:, 1:] - ts[:, :-1]
for i, nm in enumerate(["load keys", "threshold bit search (16 rounds)", "membership scans + list", "order (rank sort)", "idx store + fused gather"]):
    print(f"  select: {nm:36s} mean {dd[:, i].mean():9.1f} max {dd[:, i].max():9.1f}")
print("  select total", float((ts[:, 5] - ts[:, 0]).mean()))
