"""Graph-replayed decoding against the host-issued step: us per generated token of a 32-layer model with Llama-3-8B head geometry
(32 query heads over 8 KV heads, D 128, hidden 4096, a small MLP as in the tests), bf16, bsz 1, one token per step, at
(prefix rows, tail rows) = (136, 64), (136, 1024), (2056, 64), (2056, 1024).  Three variants alternate in rounds in one process, HIP
events around `reps` steps each, the median round is reported:
  (a) GraphDecoder: one graph replay per token (kvc_decode_step_dev inside);
  (b) GraphDecoder(capture=False): the same kernels and books issued eagerly;
  (c) the path without this feature: the eager model step over kvc_decode_step2 (model(tok, past_key_values=DynamicCache)).
Every variant is put at the point directly — the prompt is compressed to the prefix length by SnapKV, the tail is set to random rows
and its length written into the mirrors and the device counter — and set back to it after every timed window, so that all three
see the same lengths in every round.  (a) and (b) run with a tail capacity of `factor` x tail rows (2 and 8): the grid of their
attention kernel is sized from prefix + capacity, not from the rows in use.
Gate: (a) <= (c) at every point and capacity.  (b) - (c) is the price of the bound-sized grid when issued eagerly (no gate).
Prints one JSON object per point and, with --out FILE, appends them to FILE.  --quick: two points, fewer repetitions (for a kernel
trace run under rocprofv3).  Exit status 1 when the gate fails."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transformers import DynamicCache, LlamaConfig, LlamaForCausalLM

from kvcache_factory_amd import GraphDecoder, monkeypatch

dev = torch.device("cuda:0")
QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
LAYERS, W = 32, 8
POINTS = ((136, 64), (2056, 1024)) if QUICK else ((136, 64), (136, 1024), (2056, 64), (2056, 1024))
FACTORS = (2, 8)
REPS, ROUNDS = (8, 3) if QUICK else (32, 9)


def build():
    monkeypatch.replace_llama("snapkv")
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=256, num_hidden_layers=LAYERS, num_attention_heads=32, num_key_value_heads=8,
                      head_dim=128, vocab_size=256, max_position_embeddings=8192, attn_implementation="sdpa", eos_token_id=None,
                      pad_token_id=0, bos_token_id=None)
    torch.manual_seed(0)
    with torch.device(dev):                                                  # (weights drawn on the device: 1.4 G parameters)
        model = LlamaForCausalLM(cfg)
    return model.to(torch.bfloat16).eval()


def set_prefix(model, rows):
    for layer in model.model.layers:
        for name, val in (("window_size", W), ("max_capacity_prompt", rows), ("kernel_size", 7), ("pooling", "maxpool")):
            setattr(layer.self_attn.config, name, val)


def events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


class Decoder:
    """GraphDecoder at (P, T): the tails hold T random rows, mirrors and counter say T; `rewind` puts it back there."""

    def __init__(self, model, ids, T, capacity, capture):
        self.dec, self.T, self.L = GraphDecoder(model, tail_rows=capacity, capture=capture), T, ids.shape[1]
        self.tok = self.dec.prefill(ids)[:, -1].argmax(-1, keepdim=True)
        for layer in self.dec._cache.layers:
            layer._ktail.normal_()
            layer._vtail.normal_()
        self.rewind()
        self.step()                                                          # the capture, the workspaces
        self.rewind()

    def rewind(self):
        d = self.dec
        d._counter.fill_(self.T)
        d._pos.fill_(self.L + self.T)
        d._tail = self.T
        for layer in d._cache.layers:
            layer._tail, layer.true_length = self.T, self.L + self.T

    def step(self):
        self.dec.step(self.tok)


class Today:
    """The eager model step over kvc_decode_step2 at the same point (the layers' own SPLIT form, tail set to T random rows)."""

    def __init__(self, model, ids, T, reps):
        self.model, self.T, self.L = model, T, ids.shape[1]
        self.cache = DynamicCache()
        with torch.no_grad():
            self.tok = model(ids, past_key_values=self.cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
            self.step()                                                      # into the SPLIT form
        for layer in self.cache.layers:
            b, hkv, _, d = layer._ktail.shape
            layer._ktail = torch.randn(b, hkv, T + reps + 8, d, device=dev).to(layer._ktail.dtype)
            layer._vtail = torch.randn_like(layer._ktail)
        self.rewind()
        self.step()
        self.rewind()

    def rewind(self):
        for layer in self.cache.layers:
            layer._tail, layer.true_length = self.T, self.L + self.T

    def step(self):
        with torch.no_grad():
            self.model(self.tok, past_key_values=self.cache, use_cache=True)


def point(model, P, T, factor):
    set_prefix(model, P)
    ids = torch.randint(1, 256, (1, P + 200), generator=torch.Generator().manual_seed(P)).to(dev)
    variants = [Decoder(model, ids, T, factor * T, True), Decoder(model, ids, T, factor * T, False), Today(model, ids, T, REPS)]
    assert all(layer._stored == P for v in variants[:2] for layer in v.dec._cache.layers) and REPS <= (factor - 1) * T
    torch.cuda.synchronize()
    rounds = []
    for _ in range(ROUNDS):
        row = []
        for v in variants:
            row.append(events_us(v.step, REPS))
            v.rewind()
        rounds.append(row)
    a, b, c = (statistics.median(r[i] for r in rounds) for i in range(3))
    assert variants[0].dec.captures == 1 and variants[0].dec.grows == 0
    return dict(measure="graph_decode", layers=LAYERS, prefix_rows=P, tail_rows=T, tail_capacity=factor * T, reps=REPS, rounds=ROUNDS,
                us_per_token_a_replay=round(a, 1), us_per_token_b_eager_dev=round(b, 1), us_per_token_c_today=round(c, 1),
                b_minus_c_us=round(b - c, 1), a_over_c=round(a / c, 3), gate_a_le_c=bool(a <= c),
                spread_a_us=[round(min(r[0] for r in rounds), 1), round(max(r[0] for r in rounds), 1)],
                spread_c_us=[round(min(r[2] for r in rounds), 1), round(max(r[2] for r in rounds), 1)])


def main():
    model = build()
    ok = True
    for P, T in POINTS:
        for factor in FACTORS:
            line = json.dumps(point(model, P, T, factor))
            print(line, flush=True)
            if OUT:
                with open(OUT, "a") as f:
                    f.write(line + "\n")
            ok = ok and json.loads(line)["gate_a_le_c"]
    monkeypatch.replace_llama("fullkv")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
