"""us per 32-layer launch of the window-8 softmax + pool stage alone, its two forms alternating in ONE process:
  pair : softmax_pool_pair_kernel (two heads per CU; exponentials recomputed in pass 2)      debug_stage_mask 6
  keep : softmax_pool_ws_kernel (one head per CU; exponentials kept in registers)            debug_stage_mask 6 | 1 << 14
The benchmark's geometry (C2: 32 layers x 32 query heads, L = 8000, bf16, SnapKV 8k -> 128, torch_cpu ties): one BatchPlan,
run once so that the logits are in its workspace; then ROUNDS rounds per form, each LAUNCHES launches between two HIP
events, as bench.py's kernel_breakdown times a stage.  Prints every round, then one JSON object.
    python3 tools/softmax_pair_timing.py [rounds >= 5] [launches >= 20]"""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from kvcache_factory_amd import _kvc, synth

ROUNDS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
LAUNCHES = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 50
HQ, HKV, D, LAYERS, L, W, CAP = 32, 8, 128, 32, 8000, 8, 128
FORMS = (("pair", 6), ("keep", 6 | 1 << 14))
dev = torch.device("cuda:0")
qkv = [synth.make_qkv(HQ, HKV, L, D, torch.bfloat16, l, device=dev) for l in range(LAYERS)]
bp = _kvc.BatchPlan(_kvc.SNAPKV, qkv, W, [CAP - W] * LAYERS, 7, "maxpool", "torch_cpu", want_indices=True)
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
bp.run(stream)                                                   # the logits now exist
torch.cuda.synchronize(dev)


def one_round(mask):
    pp = _kvc.Params.from_buffer_copy(bp.p)
    pp.debug_stage_mask = mask
    assert bp.call(params=pp, stream=stream) == 0, _kvc.lib().kvc_last_error()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        bp.call(params=pp, stream=stream)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES


for _, mask in FORMS:                                            # warm-up: both kernels loaded, their LDS limits set
    one_round(mask)
us = {name: [] for name, _ in FORMS}
for r in range(ROUNDS):
    for name, mask in FORMS:
        us[name].append(round(one_round(mask), 2))
        print("round %d %s %.2f us" % (r, name, us[name][-1]), flush=True)
med = {name: statistics.median(v) for name, v in us.items()}
print(json.dumps({"geometry": "32 items x 32 heads, L 8000, W 8, bf16, maxpool 7", "unit": "us per 32-layer launch of the stage",
                  "launches_per_round": LAUNCHES, "rounds": us, "median_us": med,
                  "spread_us": {name: round(max(v) - min(v), 2) for name, v in us.items()},
                  "pair_over_keep": round(med["pair"] / med["keep"], 3), "device": torch.cuda.get_device_name(0)}))
