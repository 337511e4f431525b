"""The quantized cache under graph replay against its host-issued step: us per generated token of a 32-layer model with Llama-3-8B
head geometry (32 query heads over 8 KV heads, D 128, hidden 4096, a small MLP as in the tests), bf16, bsz 1, one token per step,
G 64, R 128, at prefix rows 136 and 2 056, 0 and 1 024 rows in use on the quantized tail, a tail capacity of 1 x and 2 x the rows in
use (128 rows when none are), 2 / 4 / 8 bits.  Four variants alternate in rounds in one process, HIP events around `reps` steps each,
the median round is reported:
  (a) GraphDecoder(nbits=N): one graph replay per token (kvc_decode_step_quant_dev inside);
  (b) GraphDecoder(nbits=N, capture=False): the same kernels and books issued eagerly;
  (c) the path without this feature: the eager model step over QuantizedCompressedCache (kvc_decode_step_quant);
  (d) plain bf16 replay, GraphDecoder(model), at the same rows.
Every variant is put at the point directly — the prompt is compressed to the prefix length by SnapKV, the tail is set to random
codes / rows and its length written into the mirrors and the device words — and set back to it after every timed window (the
residual starts empty and takes the window's rows: no flush inside a window).
Gate: (a) <= (c) at every point.  (a) against (d) is reported, not gated.
Prints one JSON object per point and, with --out FILE, appends them to FILE.  --quick: two points, one width, fewer repetitions (for
a kernel trace run under rocprofv3).  Exit status 1 when the gate fails."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transformers import LlamaConfig, LlamaForCausalLM

from kvcache_factory_amd import GraphDecoder, QuantizedCompressedCache, monkeypatch

dev = torch.device("cuda:0")
QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
LAYERS, W, G, R = 32, 8, 64, 128
POINTS = ((136, 0), (2056, 1024)) if QUICK else ((136, 0), (136, 1024), (2056, 0), (2056, 1024))
WIDTHS = (4,) if QUICK else (2, 4, 8)
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


def random_segment(bufs):
    """Finite contents for a quantized segment: any codes, scales of about 0.01, zeros of about -1."""
    kc, vc, km, vm = bufs
    kc.random_(0, 256)
    vc.random_(0, 256)
    km.uniform_(0.005, 0.02)
    km[:, :, :, 1].uniform_(-1.5, -0.5)
    vm.uniform_(0.005, 0.02)
    vm[..., 1].uniform_(-1.5, -0.5)


class Quant:
    """GraphDecoder(nbits=...) at (P, Tq): the tails hold Tq rows of random codes, mirrors and words say (Tq, 0)."""

    def __init__(self, model, ids, nbits, Tq, capacity, capture):
        self.dec = GraphDecoder(model, nbits=nbits, q_group_size=G, residual_length=R, tail_rows=capacity, capture=capture)
        self.Tq, self.L = Tq, ids.shape[1]
        self.tok = self.dec.prefill(ids)[:, -1].argmax(-1, keepdim=True)
        for layer in self.dec._cache.layers:
            random_segment(layer.segments()[1][:4])
        self.rewind()
        self.step()                                                          # the capture, the workspaces
        self.rewind()

    def rewind(self):
        d = self.dec
        d._counter[0].fill_(self.Tq)
        d._counter[1].zero_()
        d._pos.fill_(self.L + self.Tq)
        d._tail = self.Tq
        for layer in d._cache.layers:
            layer._trows, layer._rrows, layer.true_length = self.Tq, 0, self.L + self.Tq

    def step(self):
        self.dec.step(self.tok)


class Plain:
    """GraphDecoder(model) — the bf16 cache — at the same rows: a tail of T random rows."""

    def __init__(self, model, ids, T, capacity):
        self.dec, self.T, self.L = GraphDecoder(model, tail_rows=capacity), T, ids.shape[1]
        self.tok = self.dec.prefill(ids)[:, -1].argmax(-1, keepdim=True)
        for layer in self.dec._cache.layers:
            layer._ktail.normal_()
            layer._vtail.normal_()
        self.rewind()
        self.step()
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
    """The eager model step over QuantizedCompressedCache at the same point (the layers' fused form, the tail set to Tq rows)."""

    def __init__(self, model, ids, nbits, Tq):
        self.model, self.Tq, self.L = model, Tq, ids.shape[1]
        self.cache = QuantizedCompressedCache(model.config, nbits=nbits, q_group_size=G, residual_length=R)
        with torch.no_grad():
            self.tok = model(ids, past_key_values=self.cache, use_cache=True).logits[:, -1].argmax(-1, keepdim=True)
            self.step()                                                      # into the fused form: the prompt is quantized
        if Tq:
            for layer in self.cache.layers:
                layer._grow_tail(Tq)
                random_segment((layer._tkc, layer._tvc, layer._tkm, layer._tvm))
        self.rewind()
        self.step()
        self.rewind()

    def rewind(self):
        for layer in self.cache.layers:
            layer._trows, layer._rrows, layer.true_length = self.Tq, 0, self.L + self.Tq

    def step(self):
        with torch.no_grad():
            self.model(self.tok, past_key_values=self.cache, use_cache=True)


def point(model, P, Tq, factor, nbits):
    set_prefix(model, P)
    ids = torch.randint(1, 256, (1, P + 200), generator=torch.Generator().manual_seed(P)).to(dev)
    capacity = max(R, factor * Tq)
    variants = [Quant(model, ids, nbits, Tq, capacity, True), Quant(model, ids, nbits, Tq, capacity, False), Today(model, ids, nbits, Tq),
                Plain(model, ids, Tq, capacity + R)]
    assert all(layer.rows()[0] == P for v in variants[:2] for layer in v.dec._cache.layers) and REPS < R
    torch.cuda.synchronize()
    rounds = []
    for _ in range(ROUNDS):
        row = []
        for v in variants:
            row.append(events_us(v.step, REPS))
            v.rewind()
        rounds.append(row)
    a, b, c, d = (statistics.median(r[i] for r in rounds) for i in range(4))
    assert variants[0].dec.captures == 1 and variants[0].dec.grows == 0 and variants[3].dec.captures == 1
    return dict(measure="quant_graph", layers=LAYERS, nbits=nbits, prefix_rows=P, quant_tail_rows=Tq, tail_capacity=capacity, reps=REPS,
                rounds=ROUNDS, us_per_token_a_replay=round(a, 1), us_per_token_b_eager_dev=round(b, 1), us_per_token_c_today=round(c, 1),
                us_per_token_d_bf16_replay=round(d, 1), a_over_c=round(a / c, 3), a_over_d=round(a / d, 3), gate_a_le_c=bool(a <= c),
                spread_a_us=[round(min(r[0] for r in rounds), 1), round(max(r[0] for r in rounds), 1)],
                spread_c_us=[round(min(r[2] for r in rounds), 1), round(max(r[2] for r in rounds), 1)])


def main():
    model = build()
    ok = True
    for P, Tq in POINTS:
        for factor in ((1, 2) if Tq else (1,)):
            for nbits in WIDTHS:
                line = json.dumps(point(model, P, Tq, factor, nbits))
                print(line, flush=True)
                if OUT:
                    with open(OUT, "a") as f:
                        f.write(line + "\n")
                ok = ok and json.loads(line)["gate_a_le_c"]
    monkeypatch.replace_llama("fullkv")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
