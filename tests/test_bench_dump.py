"""bench.py --dump-outputs on CPU tensors shaped like C2's: what the last timed step handed its caller, within 64 MB,
the same sample positions on every run, written whole where it fits."""
import os

import numpy as np
import torch

import bench


class _Outputs:
    """Stands in for a resident prompt of bench.Prompt: per-layer K', V' and kept indices."""

    def __init__(self, keeps, seed, W=8, L=8000):
        g = torch.Generator().manual_seed(seed)
        self.k = [torch.randn(1, 32, kk + W, 128, generator=g).to(torch.bfloat16) for kk in keeps]
        self.v = [torch.randn(1, 32, kk + W, 128, generator=g).to(torch.bfloat16) for kk in keeps]
        self.i = [torch.randint(0, L - W, (1, 32, kk), generator=g) for kk in keeps]

    def outputs(self):
        return self.k, self.v, self.i


def test_dump_outputs_budget_and_repeatability(tmp_path):
    prompts = [_Outputs([120] * 32, s) for s in range(2)]
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(prompts, [0, 1], str(a))
    bench.dump_outputs(prompts, [0, 1], str(b))
    files = sorted(os.listdir(a))
    assert files == [f"set{s}_{n}.npy" for s in (0, 1) for n in ("indices", "k_out", "v_out")]
    assert sum(os.path.getsize(a / f) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
    idx = np.load(a / "set1_indices.npy")                    # 122 880 indices: written whole, exactly
    assert np.array_equal(idx, torch.cat([t.reshape(-1) for t in prompts[1].i]).double().numpy())
    k = np.load(a / "set0_k_out.npy")                        # 16.8 M elements over the 32 layers: a sample of them
    full = torch.cat([t.reshape(-1) for t in prompts[0].k]).float().numpy()
    assert 0 < k.size < full.size and np.isin(k, full).all()
