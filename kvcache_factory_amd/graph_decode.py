"""Graph-replayed decoding: one whole model step captured in a HIP graph and replayed for every generated token.

A host-issued decode step costs more host time than kernel time (~24 us per layer for ~10 us of kernels).
What kept a step from being captured was that the tail length was a host integer in the kernel arguments, the grid and the split
plan.  kvc_decode_step_dev reads it on the device, the layers' device-length mode (cache.CompressedDynamicLayer) gives the tail a
fixed capacity and a workspace of its own, and this class owns what is left: static input buffers, the device counter every
layer reads, the capture, the host mirror of the lengths and the growth of the tails.

    monkeypatch.replace_llama("snapkv")              # pyramidkv, streamingllm, h2o, l2norm, cam alike; replace_mistral too
    dec = GraphDecoder(model, tail_rows=256)         # capture=False: the same kernels and books, issued eagerly
    logits = dec.prefill(input_ids, attention_mask)  # eager, through the patched forwards
    logits = dec.step(tokens)                        # tokens [bsz, 1] on the device -> the static logits buffer [bsz, 1, vocab]
    out = dec.generate(input_ids, max_new_tokens=64) # greedy; argmax on the device, no host read per token

The captured region is ONE chain on ONE stream: the model step, the copy of its logits into the static buffer and two in-graph
`add_`s that advance the tail counter and the positions.  When the mirror says the tails are full, every layer's tail is doubled
and the step is captured again: O(log n) captures, decided by host arithmetic.  `step` returns the static buffer — it is
overwritten by the next step, so a caller who keeps logits clones them.

    dec = GraphDecoder(model, interval=128)          # snapkv, pyramidkv, streamingllm; one sequence

bounds every layer while it replays: DecodeCompressedCache's budget and trigger on cache.BoundedDeviceLayer, whose buffers keep their
addresses for the whole generation.  The tails never grow, so ONE capture serves however many tokens follow; every layer has its
own device counter (one int32 vector, advanced by one in-graph add), and after a step the host mirrors decide, layer by layer,
whether a compression runs — eagerly, between two replays, on the same stream.  `tail_rows` is not used in this mode.

    monkeypatch.replace_llama("h2o")
    dec = GraphDecoder(model, heavy_hitter=128)      # h2o only; one sequence

is the same for H2O's own decode-time rule (HeavyHitterCache's): the prompt goes through an internal HeavyHitterCache, every layer is
then a cache.BoundedHeavyHitterLayer whose captured step (kvc_decode_step_dev_scored) accumulates the scores, and every `heavy_hitter`
tokens the mirrors have each layer evict its lowest-scoring rows between two replays.  One capture, no growth, no host read.

    dec = GraphDecoder(model, nbits=4, q_group_size=64, residual_length=128, tail_rows=1024)      # one sequence

replays the quantized (KIVI-style) cache, QuantizedCompressedCache's rule on cache.QuantizedDeviceLayer: the prompt is quantized once
when the layers are adopted, the captured step (kvc_decode_step_quant_dev) reads the rows of the quantized tail and of the residual
from two device words per layer, and an in-graph add advances the residual words.  Every `residual_length` tokens the mirrors have
each layer quantize its residual onto the tail between two replays; `tail_rows` (rounded up to a multiple of `residual_length`) is the
tail's first capacity, doubled — with a new capture — when the next flush would not fit.
"""
import torch

from . import pyramidkv_utils as pu
from .cache import (DECODE_METHODS, BoundedDeviceLayer, BoundedHeavyHitterLayer, CompressedDynamicLayer, DecodeCompressedCache,
                    HeavyHitterCache, HeavyHitterLayer, QuantizedCompressedCache, QuantizedDeviceLayer, _check_interval,
                    _check_quant_args, decode_budget, heavy_hitter_budget)

_OWN_LAYOUT = ("adakv", "headkv", "think")


def _on_gpu(t):
    return t.is_cuda


def tails_needed(capacity, tail, t):
    """How often a tail of `capacity` rows holding `tail` must double before a step of t rows fits (host arithmetic)."""
    n = 0
    while tail + t > capacity:
        capacity, n = 2 * capacity, n + 1
    return n


class GraphDecoder:
    WARMUP = 2                          # eager steps of the same code before a capture (lazy initialisations, workspaces, plans)

    def __init__(self, model, tail_rows=256, capture=True, interval=None, heavy_hitter=None, nbits=None, q_group_size=64,
                 residual_length=128):
        if isinstance(tail_rows, bool) or not isinstance(tail_rows, int) or tail_rows < 1:
            raise ValueError(f"tail_rows must be an int >= 1, got {tail_rows!r}")
        if interval is not None:
            _check_interval(interval)
        if heavy_hitter is not None:
            if isinstance(heavy_hitter, bool) or not isinstance(heavy_hitter, int) or heavy_hitter < 1:
                raise ValueError(f"heavy_hitter must be an int >= 1, got {heavy_hitter!r}")
            if interval is not None:
                raise ValueError("kvcache_factory_amd: GraphDecoder takes interval= (snapkv / pyramidkv / streamingllm) or "
                                 "heavy_hitter= (h2o), not both")
        if nbits is not None:
            _check_quant_args(nbits, q_group_size, residual_length)
            if interval is not None or heavy_hitter is not None:
                raise ValueError("kvcache_factory_amd: GraphDecoder takes nbits= (the quantized cache) or interval= / heavy_hitter= "
                                 "(a bounded cache), not both")
            tail_rows = -(-tail_rows // residual_length) * residual_length   # the quantized tail takes whole residuals
        self.model, self.tail_rows, self.capture, self.interval, self.heavy_hitter = model, tail_rows, bool(capture), interval, heavy_hitter
        self.nbits, self.q_group_size, self.residual_length = nbits, q_group_size, residual_length
        self.config = model.config.get_text_config() if hasattr(model.config, "get_text_config") else model.config
        self._refuse_model()
        self._clusters()
        self._refuse_quant()
        self.captures = 0               # graphs captured since the last prefill
        self.grows = 0                  # times the tails were doubled since the last prefill
        self._cache = self._graph = None
        self._layers = ()
        self._tok = self._pos = self._logits = self._counter = self._stepped = None

    # ---- refusals: all raised before anything is stored or captured --------------------------------------------------------------
    def _attn(self):
        return self.model.model.layers[0].self_attn

    def _refuse_model(self):
        attn = self._attn()
        method = getattr(type(attn).forward, "kvc_method", None)
        if method is None:
            raise NotImplementedError("kvcache_factory_amd: GraphDecoder needs a model whose attention was patched by "
                                      "monkeypatch.replace_llama / replace_mistral before it was built; this model is unpatched "
                                      "(fullkv keeps no compressed cache to decode over)")
        if method in _OWN_LAYOUT:
            raise NotImplementedError(f"kvcache_factory_amd: {method} keeps a cache layout of its own (ragged heads / pruned channels); "
                                      "graph-replayed decoding covers the plain compressed cache only")
        if getattr(self.config, "sliding_window", None) is not None:
            raise NotImplementedError("kvcache_factory_amd: the fused decode step has no sliding window "
                                      f"(sliding_window={self.config.sliding_window}); GraphDecoder cannot replay this model")
        if getattr(self.config, "output_attentions", False):
            raise NotImplementedError("kvcache_factory_amd: output_attentions needs the reference-shaped attention; the fused decode "
                                      "step returns no weights, so GraphDecoder refuses it")
        if attn.head_dim not in (64, 128):
            raise NotImplementedError(f"kvcache_factory_amd: the decode kernels are built for head_dim 64 and 128, got {attn.head_dim}")
        if self.model.training:
            raise NotImplementedError("kvcache_factory_amd: GraphDecoder decodes in eval mode only (the fused step has no dropout)")
        self.method = method

    def _clusters(self):
        """interval / heavy_hitter mode: every layer's kv_cluster as the patched forward builds it from the config now, through the
        mode's budget rule — a method without the rule and merge="pivot" are NotImplementedError, a period < window_size a ValueError."""
        from .attention import _INIT
        if self.heavy_hitter is not None:
            if self.method != "h2o":
                raise NotImplementedError(f"kvcache_factory_amd: GraphDecoder(heavy_hitter=...) evicts by H2O's accumulated attention; "
                                          f"{self.method} has no such rule here — it is built for the h2o path only")
            clusters = []
            for block in self.model.model.layers:
                _INIT[self.method](block.self_attn)
                clusters.append(block.self_attn.kv_cluster)
                heavy_hitter_budget(clusters[-1], self.heavy_hitter)
            return clusters
        if self.interval is None:
            return None
        if self.method not in DECODE_METHODS:
            raise NotImplementedError(f"kvcache_factory_amd: {self.method} has no decode-time compression rule here; "
                                      "GraphDecoder(interval=...) is built for the snapkv / pyramidkv / streamingllm paths only")
        clusters = []
        for block in self.model.model.layers:
            _INIT[self.method](block.self_attn)
            clusters.append(block.self_attn.kv_cluster)
            decode_budget(clusters[-1], self.interval)
        return clusters

    def _refuse_quant(self):
        """nbits mode: the pivot merge has no quantized decode cache here (every layer's kv_cluster as the patched forward builds it)."""
        if self.nbits is None:
            return
        from .attention import _INIT
        for block in self.model.model.layers:
            _INIT[self.method](block.self_attn)
            merge = getattr(block.self_attn.kv_cluster, "merge", None)
            if merge is not None:
                raise NotImplementedError(f"kvcache_factory_amd: {self.method} with merge={merge!r} is not replayed over the quantized "
                                          "cache; GraphDecoder(nbits=...) needs merge=None")

    def _refuse_call(self, input_ids, cache):
        for kind, why in ((QuantizedCompressedCache, "a quantized cache (QuantizedCompressedCache / KVQuantCompressedCache) quantizes "
                                                     "its tail on a host-counted schedule"),
                          (DecodeCompressedCache, "DecodeCompressedCache re-compresses on a host-counted schedule"),
                          (HeavyHitterCache, "HeavyHitterCache evicts on a host-counted schedule")):
            if isinstance(cache, kind):
                raise NotImplementedError(f"kvcache_factory_amd: GraphDecoder replays the plain compressed cache only; {why}")
        self._refuse_model()
        if not pu.DECODE_KERNEL:
            raise NotImplementedError("kvcache_factory_amd: KVC_DECODE_KERNEL=0 turns the fused decode step off; there is nothing for "
                                      "GraphDecoder to replay")
        if input_ids.dim() != 2:
            raise ValueError("input_ids must be [bsz, length]")
        if input_ids.shape[0] > 1 and not pu.BATCH_DECODE:
            raise NotImplementedError("kvcache_factory_amd: KVC_BATCH_DECODE=0 turns the fused step off for batches; GraphDecoder "
                                      f"cannot replay a batch of {input_ids.shape[0]}")
        param = next(self.model.parameters())
        if not _on_gpu(input_ids) or not _on_gpu(param):
            raise NotImplementedError("kvcache_factory_amd: GraphDecoder runs on the GPU only (HIP kernels); got "
                                      f"input_ids on {input_ids.device} and a model on {param.device}")
        if param.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise NotImplementedError(f"kvcache_factory_amd: the decode kernels take bf16, fp16 and fp32, not {param.dtype}")

    # ---- prefill -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill(self, input_ids, attention_mask=None, past_key_values=None):
        """The prompt through the patched forwards (eager) on a fresh cache; every layer then goes into device-length mode with a
        tail of `tail_rows` (interval mode: is replaced by a BoundedDeviceLayer that takes over its rows).  Left-padded batches as the
        patched forwards take them.  -> logits [bsz, 1, vocab] of the last token."""
        from transformers import DynamicCache
        from .attention import _pending_for
        self._refuse_call(input_ids, past_key_values)
        clusters = self._clusters()
        self._refuse_quant()
        heavy, quant = self.heavy_hitter is not None, self.nbits is not None
        if quant:
            if past_key_values is not None:
                raise ValueError("kvcache_factory_amd: GraphDecoder(nbits=...) builds its own quantized cache; past_key_values must "
                                 f"be None, got a {type(past_key_values).__name__}")
            if input_ids.shape[0] != 1:
                raise NotImplementedError("kvcache_factory_amd: the fused quantized step has no batched form; "
                                          f"GraphDecoder(nbits=...) decodes one sequence, got a batch of {input_ids.shape[0]}")
        if clusters is not None:
            mode = "heavy_hitter" if heavy else "interval"
            if past_key_values is not None:
                raise ValueError(f"kvcache_factory_amd: GraphDecoder({mode}=...) builds its own bounded cache; past_key_values must "
                                 f"be None, got a {type(past_key_values).__name__}")
            if input_ids.shape[0] != 1:
                what = "H2O's decode-time eviction" if heavy else "decode-stage compression"
                raise NotImplementedError(f"kvcache_factory_amd: {what} has no per-row form; "
                                          f"GraphDecoder({mode}=...) decodes one sequence, got a batch of {input_ids.shape[0]}")
        if heavy:                                                            # the patched forward's prefill_heavy_hitter path, unchanged
            cache = HeavyHitterCache(self.model.config, self.heavy_hitter)
        else:
            cache = DynamicCache(config=self.model.config) if past_key_values is None else past_key_values
        if cache.get_seq_length() != 0:
            raise RuntimeError("kvcache_factory_amd: GraphDecoder.prefill starts from an empty cache")
        self._graph = self._cache = None
        self._layers = ()
        bsz, length = input_ids.shape
        dev = input_ids.device
        if attention_mask is None:
            position_ids = None
            pos = torch.full((bsz, 1), length, dtype=torch.long, device=dev)
        else:
            position_ids = (attention_mask.cumsum(-1) - 1).clamp(min=0)
            pos = attention_mask.sum(-1, keepdim=True).to(torch.long)         # row b goes on from its own prompt's length
        out = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, past_key_values=cache,
                         use_cache=True, logits_to_keep=1)
        _pending_for(cache).settle()
        layers = tuple(cache.layers)
        kind = HeavyHitterLayer if heavy else CompressedDynamicLayer
        for layer in layers:
            if type(layer) is not kind or not layer.can_split():
                raise NotImplementedError(f"kvcache_factory_amd: GraphDecoder found a {type(layer).__name__} in the cache after the "
                                          "prefill; graph-replayed decoding covers the plain compressed cache only")
        if quant:                                                            # two words per layer: [0] tail rows, [1] residual rows
            self._counter = torch.zeros(2, len(layers), dtype=torch.int32, device=dev)
            self._stepped = self._counter[1]                                 # one vector for the in-graph add
            cfg = self.config
            layers = tuple(QuantizedDeviceLayer.adopt(layer, self.nbits, self.q_group_size, self.residual_length, self.tail_rows,
                                                      self._counter[0, i:i + 1], self._counter[1, i:i + 1], cfg.num_key_value_heads)
                           for i, layer in enumerate(layers))
            cache.layers[:] = layers
        elif clusters is None:
            self._counter = torch.zeros(1, dtype=torch.int32, device=dev)
            for layer in layers:
                layer.enter_device_length(self._counter, self.tail_rows, self.config.num_key_value_heads)
                layer.hold_mirror(True)
        else:                                                                # one counter per layer, one vector for the in-graph add
            self._counter = torch.zeros(len(layers), dtype=torch.int32, device=dev)
            twin, period = (BoundedHeavyHitterLayer, self.heavy_hitter) if heavy else (BoundedDeviceLayer, self.interval)
            layers = tuple(twin.adopt(layer, cl, period, self._counter[i:i + 1], self.config.num_key_value_heads)
                           for i, (layer, cl) in enumerate(zip(layers, clusters)))
            cache.layers[:] = layers
        if not quant:
            self._stepped = self._counter                                    # what a step advances: every word
        self._cache, self._layers = cache, layers
        self._tok = torch.zeros(bsz, 1, dtype=torch.long, device=dev)
        self._pos = pos.contiguous()
        self._logits = out.logits.clone()
        self._tail, self._capacity = 0, layers[0].tail_capacity()
        self.captures = self.grows = 0
        return self._logits

    # ---- one step ----------------------------------------------------------------------------------------------------------------
    def _body(self):
        """The step every variant runs: model over the static buffers, logits to the static buffer, counter and positions on."""
        out = self.model(input_ids=self._tok, position_ids=self._pos, past_key_values=self._cache, use_cache=True)
        self._logits.copy_(out.logits)
        self._stepped.add_(1)
        self._pos.add_(1)

    def _capture(self):
        """WARMUP eager steps whose effect is taken back (the row they append at T is the row the real step overwrites; counter and
        positions are set back on the device, and so are the scores of a heavy-hitter layer), then ONE capture of the same body on one
        stream."""
        side = torch.cuda.Stream(self._tok.device)
        side.wait_stream(torch.cuda.current_stream(self._tok.device))
        with torch.cuda.stream(side):
            kept = [layer.scores_state() for layer in self._layers] if self.heavy_hitter is not None else ()
            for _ in range(self.WARMUP):
                self._body()
                self._stepped.sub_(1)
                self._pos.sub_(1)
            for layer, state in zip(self._layers, kept):                     # (heavy_hitter: a warm-up step also added to the scores)
                layer.set_scores_state(state)
        torch.cuda.current_stream(self._tok.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._body()                                                     # (records only: nothing ran, nothing to take back)
        self._graph = graph
        self.captures += 1

    def _grow(self):
        for layer in self._layers:
            layer.grow_tail()
        self._capacity = self._layers[0].tail_capacity()
        self._graph = None
        self.grows += 1

    @torch.no_grad()
    def step(self, tokens):
        """tokens [bsz, 1] (device) -> the static logits buffer [bsz, 1, vocab].  No host read; a graph replay when capture=True."""
        if self._cache is None:
            raise RuntimeError("kvcache_factory_amd: GraphDecoder.step before prefill")
        if self.interval is None and self.heavy_hitter is None and self.nbits is None:
            for _ in range(tails_needed(self._capacity, self._tail, 1)):
                self._grow()
        self._tok.copy_(tokens.reshape(self._tok.shape))
        if self.capture:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        else:
            self._body()
        self._tail += 1
        for layer in self._layers:                                           # the mirrors follow (no Python of the layers ran)
            layer.advance(1)
        if self.nbits is not None:
            grew = [layer.maybe_flush()[1] for layer in self._layers]        # host arithmetic; a flush is enqueued eagerly
            if any(grew):                                                    # (every layer at once: they share R and the schedule)
                self._capacity = self._layers[0].tail_capacity()
                self._graph = None
                self.grows += 1
        elif self.interval is not None:
            for layer in self._layers:                                       # host arithmetic; a compression is enqueued eagerly
                layer.maybe_compress()
        elif self.heavy_hitter is not None:
            for layer in self._layers:                                       # host arithmetic; an eviction is enqueued eagerly
                layer.maybe_evict()
        return self._logits

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, attention_mask=None):
        """Greedy decoding: -> [bsz, length + max_new_tokens].  The argmax stays on the device; nothing is read per token."""
        logits = self.prefill(input_ids, attention_mask)
        out = [input_ids]
        for j in range(max_new_tokens):
            tok = logits[:, -1].argmax(-1, keepdim=True)
            out.append(tok)
            if j + 1 < max_new_tokens:
                logits = self.step(tok)
        return torch.cat(out, 1)
