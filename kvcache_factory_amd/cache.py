"""Cache layer that holds a compressed prefix but reports the TRUE sequence length.

Counterpart of the reference's `past_key_value._seen_tokens = self.kv_seq_len` (llama_model.py:290) and of the
`kv_seq_len` reset in `prepare_inputs_for_generation_llama_new` (llama_model.py:2609-2612): after compression the
cache stores `cap` tokens per head, but RoPE positions / cache_position for the decode steps must continue from
the real prompt length.  transformers 5.x derives both from `layer.get_seq_length()`, so the layer keeps them apart.
"""
import torch
from transformers.cache_utils import Cache, DynamicLayer


def _placeholder_only(name):
    """Setter of the computed `keys` / `values` properties: DynamicLayer's constructor assigns None (and its stock
    lazy_initialization an empty tensor); anything else would be silently lost, so it is refused."""
    def setter(self, value):
        if value is not None and getattr(value, "numel", lambda: 1)() != 0:
            raise AttributeError(f"{type(self).__name__}.{name} is computed from the layer's own buffers; DynamicLayer operations that "
                                 "reassign it are overridden (batch reordering) or refused (crop, offload)")
    return setter


class _BatchOps:
    """The DynamicLayer operations that work by REASSIGNING keys / values (transformers 5.15: reorder_cache, batch_repeat_interleave,
    batch_select_indices — beam search, num_return_sequences, contrastive search — and offload / prefetch / reset), restated on the
    layer's own buffers.  `_batch_tensors` names the attributes that carry a batch dimension in front."""
    _batch_tensors = ()

    def _map_batch(self, fn):
        for name in self._batch_tensors:
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, fn(t))

    def reorder_cache(self, beam_idx):
        if self.get_seq_length() > 0:
            self._map_batch(lambda t: t.index_select(0, beam_idx.to(t.device)))

    def batch_repeat_interleave(self, repeats):
        if self.get_seq_length() > 0:
            self._map_batch(lambda t: t.repeat_interleave(repeats, dim=0))

    def batch_select_indices(self, indices):
        if self.get_seq_length() > 0:
            self._map_batch(lambda t: t[indices, ...])

    def offload(self):
        raise NotImplementedError("a compressed cache stays in the device buffers its kernels append to in place: no offloading")

    def prefetch(self):
        pass                                                            # never offloaded

    def lazy_initialization(self, key_states, value_states=None):
        """DynamicLayer's version also allocates two empty placeholder tensors for `keys` / `values`; here those are computed
        properties, so only the bookkeeping is kept (two allocations per layer and prompt less on the prefill path)."""
        self.dtype, self.device = key_states.dtype, key_states.device
        self.is_initialized = True

    def crop(self, *a, **kw):
        raise NotImplementedError("a compressed cache cannot be cropped by position")


class CompressedDynamicLayer(_BatchOps, DynamicLayer):
    """The compressed prompt of one layer plus the decoded tokens, in one of two forms.

    EXPANDED (the reference's form): `[bsz, H_q, stored, D]` — H_q heads like the reference's cache after repeat_kv.  The
    reference grows it by `torch.cat` on every generated token (`past_key_value.update` else-branch, llama_model.py:287-289:
    a copy of the whole [1, 32, cap + t, 128] tensor per layer per step); here the compressed prompt sits in a buffer with
    spare rows per head (doubled when exhausted) and a decode step writes its row(s) in place.  Same bytes.

    SPLIT (used by the fused decode step, `decode_attend`): the prefix `[bsz, H_q, k + W, D]` stays exactly
    where the compression kernels wrote it and the decoded tokens go to a TAIL `[bsz, H_kv, capacity, D]` — once per KV
    head, not H_q / H_kv times, with no repeat_kv and no copy of the prefix.  `keys` / `values` materialise the reference's
    view on demand (tests, tools); asking for them through `update` converts the layer to EXPANDED for good.

    PER-ROW LENGTHS (a left-padded batch of unequal prompts, pyramidkv_utils.prefill_rows): every prompt keeps what it keeps
    alone, so batch row b uses only the first rows[b] of the `_stored` = max(rows) prefix rows.  `_rows` holds rows[] on the
    DEVICE (int32 [bsz]; one of `_batch_tensors`, so beam reordering and the other batch operations carry it along without a
    host read); the host knows only `_stored` and that the rows differ (`has_holes()`).  Decoded rows
    are uniform — the batch decodes in lockstep — and follow row `_stored` (EXPANDED) or live in the tail (SPLIT): the columns
    [rows[b], _stored) of row b are HOLES.  The fused step never reads them (kvc_decode_step_rows); the reference-shaped form
    hides them with the layer's own additive mask (`decode_mask`), not with a slice of the mask transformers built for the
    padded prompt.  `keys` / `values` are the padded view, `row_lengths()` says what is real.  When every row keeps the same
    number of rows there are no holes and the layer is what it is for an unpadded batch.

    DEVICE-LENGTH MODE (graph-replayed decoding, graph_decode.GraphDecoder; the plain layer type only): the SPLIT form with a tail
    of FIXED capacity whose length lives in a device counter (int32 [1], shared by the layers of one cache) that the fused step
    reads (kvc_decode_step_dev) — nothing the host passes to a step depends on the length, so a captured step replays while the
    cache grows.  `_tail` / `true_length` are then the host's MIRROR of the counter: decode_attend advances them like any step
    unless the owner of a graph holds them (`hold_mirror`) and advances them itself (`advance`) — during a replay no Python of
    the layer runs.  The tail never re-allocates inside a step: `grow_tail` doubles it, an explicit host call between replays.
    Everything that reads the layer (keys / values, lengths, masks, the batch operations, `update` / `_expand`, which leave the
    mode) works from the mirror."""

    RESERVE = 256                       # spare rows allocated with the compressed prompt / tail rows allocated at a time

    def __init__(self):
        super().__init__()
        self.true_length = 0            # tokens the model has really seen for this layer
        self._kbuf = self._vbuf = None  # [bsz, H_q, capacity, D]
        self._stored = 0                # rows in use per head of _kbuf / _vbuf
        self._ktail = self._vtail = None    # SPLIT form: [bsz, H_kv, capacity, D]
        self._tail = 0
        self._split = False
        self._rows = None               # int32 [bsz] on the device: prefix rows in use per batch row (None: _stored for all)
        self._holes = False             # the rows of the batch keep different numbers of prefix rows
        self._padded = False            # the prompt was a left-padded batch (prefill_rows): the layer masks its own decode steps
        self._pmax = 0                  # prefix rows per head the buffers hold (= _stored until `update` appends behind them)
        self._leave_device_length()

    def _leave_device_length(self):
        self._devlen = False            # device-length mode: the tail's length is read from _dev_counter by the step
        self._dev_counter = None        # int32 [1] on the device, shared by the layers of one cache; advanced by its owner
        self._dev_ws = None             # this layer's own workspace of the step (a captured step cannot use the shared pool)
        self._dev_ws_key = None
        self._dev_hold = False          # the owner advances the mirror (`advance`), decode_attend does not

    # ---- the reference's view --------------------------------------------------------------------------------------
    # (`keys` / `values` are plain attributes of DynamicLayer; here they are computed from the buffers)
    keys = property(lambda self: self._view(self._kbuf, self._ktail), _placeholder_only("keys"))
    values = property(lambda self: self._view(self._vbuf, self._vtail), _placeholder_only("values"))
    _batch_tensors = ("_kbuf", "_vbuf", "_ktail", "_vtail", "_rows")

    def reset(self):
        """Back to an empty layer (the next forward is a prefill): buffers, lengths and the split state go."""
        self._kbuf = self._vbuf = self._ktail = self._vtail = self._rows = None
        self._stored = self._tail = self.true_length = self._pmax = 0
        self._split = self._holes = self._padded = False
        self._leave_device_length()

    def _view(self, buf, tail):
        if buf is None:
            return None
        pre = buf[:, :, :self._stored]
        if not self._split or self._tail == 0:
            return pre
        g = buf.shape[1] // tail.shape[1]
        return torch.cat([pre, tail[:, :, :self._tail].repeat_interleave(g, dim=1)], dim=2)

    # ---- prefill ------------------------------------------------------------------------------------------------------
    def _place(self, k, v, spare):
        b, h, n, d = k.shape
        kb = torch.empty(b, h, n + spare, d, dtype=k.dtype, device=k.device)
        vb = torch.empty_like(kb)
        kb[:, :, :n].copy_(k)
        vb[:, :, :n].copy_(v)
        self._kbuf, self._vbuf, self._stored = kb, vb, n

    def reserve(self, bsz, n_heads, capacity, head_dim, dtype, device):
        """Buffers [bsz, H_q, capacity, D] the compression kernels write K' / V' into directly (kvc_params.out_stride_h):
        the compressed prompt is produced in its final home, `prefill` then only records its length."""
        self._kbuf = torch.empty(bsz, n_heads, capacity, head_dim, dtype=dtype, device=device)
        self._vbuf = torch.empty_like(self._kbuf)
        self._stored = 0
        return self._kbuf, self._vbuf

    @classmethod
    def reserve_many(cls, layers, bsz, n_heads, capacities, head_dim, dtype, device):
        """`reserve` for a group of layers out of ONE allocation (the grouped flush of PrefillBatch: one torch.empty and one
        stream bookkeeping call per group instead of two per layer).  The slab lives as long as any layer's views do."""
        per = [bsz * n_heads * c * head_dim for c in capacities]
        slab = torch.empty(2 * sum(per), dtype=dtype, device=device)
        outs, off = [], 0
        for layer, c, n in zip(layers, capacities, per):
            layer._kbuf = slab[off:off + n].view(bsz, n_heads, c, head_dim)
            layer._vbuf = slab[off + n:off + 2 * n].view(bsz, n_heads, c, head_dim)
            layer._stored = 0
            outs.append((layer._kbuf, layer._vbuf))
            off += 2 * n
        return slab, outs

    def prefill(self, k_compressed, v_compressed, true_length):
        if not self.is_initialized:
            self.lazy_initialization(k_compressed, v_compressed)
        if self._kbuf is not None and k_compressed.data_ptr() == self._kbuf.data_ptr() and \
                v_compressed.data_ptr() == self._vbuf.data_ptr():      # already written into our own buffers
            self._stored = k_compressed.shape[2]
        else:
            self._place(k_compressed, v_compressed, self.RESERVE)
        self._split, self._tail, self._ktail, self._vtail = False, 0, None, None
        self._rows, self._holes, self._padded, self._pmax = None, False, False, self._stored
        self.true_length = int(true_length)
        self._leave_device_length()

    # ---- prefill of a left-padded batch: per-row lengths -----------------------------------------------------------------------
    def reserve_rows(self, bsz, n_heads, rows, head_dim, dtype, device, spare):
        """Buffers [bsz, H_q, max(rows) + spare, D] for a batch whose row b keeps rows[b] rows (host ints).  Layer types that
        cannot hold unequal rows refuse HERE, before anything is allocated or written."""
        return self.reserve(bsz, n_heads, max(rows) + spare, head_dim, dtype, device)

    def prefill_rows(self, rows, true_length):
        """Records what reserve_rows' buffers hold once the per-row compressions have run: row b its first rows[b] rows."""
        n = max(rows)
        self.prefill(self._kbuf[:, :, :n], self._vbuf[:, :, :n], true_length)
        self._padded = True
        if min(rows) != n:
            self._holes = True
            for b, r in enumerate(rows):                                # the holes are masked, but a masked NaN still poisons
                if r < n:                                               # 0 * V in the reference-shaped form: they hold zeros
                    self._kbuf[b, :, r:n].zero_()
                    self._vbuf[b, :, r:n].zero_()
            dev = self._kbuf.device
            host = torch.tensor(rows, dtype=torch.int32)
            # (a pinned source and a non-blocking copy: the prefill's only host wait is the read of the mask)
            self._rows = host.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else host

    def row_lengths(self):
        """int32 [bsz] on the layer's device: the prefix rows batch row b really holds (`keys` / `values` are padded to the
        longest).  No host read."""
        if self._kbuf is None:
            return None
        if self._rows is None:
            n = self._stored if self._split else self._pmax              # (EXPANDED: decoded rows follow the prefix in _kbuf)
            return torch.full((self._kbuf.shape[0],), n, dtype=torch.int32, device=self._kbuf.device)
        return self._rows

    def has_holes(self):
        return self._holes

    def owns_mask(self):
        """The prompt was a left-padded batch: a reference-shaped decode step takes `decode_mask`, not transformers' mask (built
        for the padded prompt's columns, which are not the rows that were kept)."""
        return self._padded

    def decode_mask(self, query_length, dtype, total=None, bsz=None):
        """The additive mask [bsz, 1, t, total] of a reference-shaped decode step over this layer AFTER `update` has appended
        the step's t rows (total: the keys `update` returned, by default this layer's own rows): 0 = attend, finfo.min on the
        hole columns [rows[b], first decoded row) of row b and on the step's own later tokens.  Every other stored row belongs
        to the prompt it is stored for.  Built on the device (from `_rows` when the rows differ)."""
        t = query_length
        total = self._stored if total is None else total
        dev = self._kbuf.device if self._kbuf is not None else self.device
        bsz = self._kbuf.shape[0] if bsz is None else bsz
        col = torch.arange(total, device=dev)
        hidden = (col[None, :] > (total - t + torch.arange(t, device=dev))[:, None])[None, None]          # [1, 1, t, total]
        if self._holes:
            hole = (col[None, :] >= self._rows[:, None].to(col.dtype)) & (col[None, :] < self._pmax)      # [b, total]
            hidden = hidden | hole[:, None, None, :]
        return torch.zeros(bsz, 1, t, total, dtype=dtype, device=dev).masked_fill(hidden, torch.finfo(dtype).min)

    # ---- decode: the reference-shaped path ----------------------------------------------------------------------------
    def _expand(self):
        """SPLIT -> EXPANDED (a caller wants plain H_q-head tensors to attend over)."""
        if self._split:
            k, v = self.keys, self.values                             # (device-length mode: the rows the mirror counts)
            self._split, self._tail, self._ktail, self._vtail = False, 0, None, None
            self._leave_device_length()
            self._place(k, v, self.RESERVE)

    def update(self, key_states, value_states, *args, **kwargs):
        """Append H_q-head rows (the caller repeat_kv-expanded them like the reference) and return the whole cache."""
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        t = key_states.shape[-2]
        self._expand()
        if self._kbuf is None:                                    # a layer that never went through prefill()
            self._place(key_states, value_states, self.RESERVE)
        else:
            if self._stored + t > self._kbuf.shape[2]:            # out of spare rows: double
                self._place(self._kbuf[:, :, :self._stored], self._vbuf[:, :, :self._stored], max(self._kbuf.shape[2], t))
            n = self._stored
            self._kbuf[:, :, n:n + t].copy_(key_states)
            self._vbuf[:, :, n:n + t].copy_(value_states)
            self._stored = n + t
        self.true_length += t
        return self.keys, self.values

    # ---- decode: the fused step ---------------------------------------------------------------------------------------
    def decode_attend(self, query_states, key_states, value_states, scaling):
        """One decode step in the SPLIT form: key_states / value_states [bsz, H_kv, t, D] are appended to the tail by the
        kernel and the attention output [bsz, t, H_q, D] over prefix + tail comes back (kvc_decode_step)."""
        from . import _kvc
        t = key_states.shape[-2]
        b, hkv, _, d = key_states.shape
        if self._devlen:
            return self._decode_attend_dev(query_states, key_states, value_states, scaling)
        if not self._split:
            self._split, self._tail = True, 0
            self._ktail = torch.empty(b, hkv, self.RESERVE, d, dtype=key_states.dtype, device=key_states.device)
            self._vtail = torch.empty_like(self._ktail)
        if self._tail + t > self._ktail.shape[2]:                 # tail full: double it
            cap = max(2 * self._ktail.shape[2], self._tail + t)
            kt = torch.empty(b, hkv, cap, d, dtype=self._ktail.dtype, device=self._ktail.device)
            vt = torch.empty_like(kt)
            kt[:, :, :self._tail].copy_(self._ktail[:, :, :self._tail])
            vt[:, :, :self._tail].copy_(self._vtail[:, :, :self._tail])
            self._ktail, self._vtail = kt, vt
        if b > 1 and type(self)._batched_step:                    # a batch: per-row prefix lengths, one launch for all rows
            if self._rows is None or self._rows.shape[0] != b:
                self._rows = self.row_lengths()
            out = _kvc.decode_step_rows(query_states, key_states, value_states, self._kbuf, self._vbuf, self._rows, self._stored,
                                        self._ktail, self._vtail, self._tail, scaling)
        else:
            out = _kvc.decode_step(query_states, key_states, value_states, self._kbuf, self._vbuf, self._stored,
                                   self._ktail, self._vtail, self._tail, scaling)
        self._tail += t
        self.true_length += t
        return out

    _batched_step = True                # bsz > 1 decode_attend calls go through kvc_decode_step_rows

    # ---- decode: the fused step with the tail length on the device (graph replay) ------------------------------------------------
    def enter_device_length(self, counter, capacity, n_kv_heads):
        """Into device-length mode: a tail [bsz, n_kv_heads, capacity, D] of fixed capacity (the rows an earlier SPLIT tail holds
        are copied) whose length the fused step reads from `counter` (int32 [1] on this layer's device).  The caller owns the
        counter: it holds this layer's `_tail` now and is advanced, in stream order, after every step."""
        if type(self) is not CompressedDynamicLayer:
            raise NotImplementedError(f"kvcache_factory_amd: {type(self).__name__} has no device-length mode (graph-replayed decoding "
                                      "covers the plain compressed cache only)")
        if self._kbuf is None:
            raise RuntimeError("kvcache_factory_amd: device-length mode needs a layer that went through a prefill")
        if not self._split and self._stored != self._pmax:
            raise NotImplementedError("kvcache_factory_amd: this layer already holds decoded rows in the reference-shaped form; enter "
                                      "device-length mode right after the prefill")
        assert counter.dtype == torch.int32 and counter.numel() == 1 and counter.device == self._kbuf.device
        b, _, _, d = self._kbuf.shape
        live = self._tail if self._split else 0
        kt = torch.empty(b, n_kv_heads, max(int(capacity), live + 1), d, dtype=self._kbuf.dtype, device=self._kbuf.device)
        vt = torch.empty_like(kt)
        if live:
            kt[:, :, :live].copy_(self._ktail[:, :, :live])
            vt[:, :, :live].copy_(self._vtail[:, :, :live])
        self._ktail, self._vtail, self._split, self._tail = kt, vt, True, live
        self._devlen, self._dev_counter, self._dev_ws, self._dev_ws_key = True, counter, None, None

    def tail_capacity(self):
        return self._ktail.shape[2] if self._split else 0

    def grow_tail(self):
        """Device-length mode: a tail of twice the capacity with the live rows copied (host arithmetic on the mirror; no device
        read).  Graphs captured over the old buffers are stale afterwards: the owner captures again."""
        assert self._devlen
        b, hkv, cap, d = self._ktail.shape
        kt = torch.empty(b, hkv, 2 * cap, d, dtype=self._ktail.dtype, device=self._ktail.device)
        vt = torch.empty_like(kt)
        kt[:, :, :self._tail].copy_(self._ktail[:, :, :self._tail])
        vt[:, :, :self._tail].copy_(self._vtail[:, :, :self._tail])
        self._ktail, self._vtail, self._dev_ws, self._dev_ws_key = kt, vt, None, None

    def hold_mirror(self, hold=True):
        """The owner of a captured step advances the host mirror itself (`advance`): decode_attend then leaves it alone, so that
        an eager step, a capture (which runs no kernel) and a replay (which runs no Python) keep the same books."""
        self._dev_hold = bool(hold)

    def advance(self, t):
        """t rows were appended by a step whose Python did not count them (a replayed graph): the host mirror follows."""
        self._tail += t
        self.true_length += t

    def _decode_attend_dev(self, query_states, key_states, value_states, scaling):
        from . import _kvc
        b, hkv, t, _ = key_states.shape
        cap = self._ktail.shape[2]
        if self._tail + t > cap:
            raise RuntimeError(f"kvcache_factory_amd: the fixed tail holds {self._tail} of {cap} rows and the step brings {t}: "
                               "grow_tail() first (device-length mode never re-allocates inside a step)")
        key = (b, t, cap, query_states.stride(), key_states.stride())
        if self._dev_ws_key != key:                                   # once per capacity: the step's own workspace
            nbytes = _kvc.decode_dev_plan(query_states, key_states, self._kbuf, self._stored, self._ktail)[1]
            self._dev_ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self._ktail.device)
            self._dev_ws_key = key
        rows = None
        if self._holes:
            if self._rows is None or self._rows.shape[0] != b:
                self._rows = self.row_lengths()
            rows = self._rows
        out = _kvc.decode_step_dev(query_states, key_states, value_states, self._kbuf, self._vbuf, self._stored, self._ktail,
                                   self._vtail, self._dev_counter, scaling, rows_b=rows, ws=self._dev_ws)
        if not self._dev_hold:
            self.advance(t)
        return out

    def can_split(self):
        """The fused decode step needs the prefix in this layer's own buffers (a layer that went through prefill)."""
        return self._kbuf is not None

    # ---- bookkeeping --------------------------------------------------------------------------------------------------
    def stored_length(self):
        if self._kbuf is None:
            return 0
        return self._stored + (self._tail if self._split else 0)

    def get_seq_length(self):
        return self.true_length

    def get_mask_sizes(self, query_length):
        # the mask must be as wide as what attention will really see: stored tokens + the new ones
        return self.stored_length() + query_length, 0

    def after_decode(self, cluster, query_states):
        """Called by the patched forwards after a decode step's attention; nothing to do unless the layer compresses at decode."""


def _uniform_rows_only(self, bsz, n_heads, rows, head_dim, dtype, device, spare):
    """reserve_rows of the layer types that only ever see K' / V' of one length per batch (decode-stage compression, the
    quantized caches): a padded batch whose prompts keep different numbers of rows is refused before anything is stored."""
    if min(rows) != max(rows):
        raise NotImplementedError(f"kvcache_factory_amd: {type(self).__name__} holds the same number of rows for every prompt of a batch; "
                                  f"this left-padded batch keeps {list(rows)} rows per prompt (prompts shorter than max_capacity_prompt "
                                  "are passed through, PyramidKV budgets follow the prompt length) — use the plain cache for it")
    return CompressedDynamicLayer.reserve_rows(self, bsz, n_heads, rows, head_dim, dtype, device, spare)


def _check_interval(interval):
    if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
        raise ValueError(f"interval must be an int >= 1, got {interval!r}")


DECODE_METHODS = ("snapkv", "pyramidkv", "streamingllm")   # the patched forwards that have a decode-time rule


def decode_budget(cluster, interval):
    """(method, B, W) of a layer compressed at decode time for `cluster` (the patched forward's kv_cluster): the one statement of
    the budget rule, shared by DecodeCompressedLayer and BoundedDeviceLayer."""
    from . import _kvc
    W = cluster.window_size
    method = cluster._method
    if method not in (_kvc.SNAPKV, _kvc.PYRAMIDKV, _kvc.STREAMINGLLM) or getattr(cluster, "merge", None) is not None:
        raise NotImplementedError(f"kvcache_factory_amd: DecodeCompressedCache has no decode-time rule for {type(cluster).__name__}"
                                  f" (merge={getattr(cluster, 'merge', None)!r})")
    if interval < W:
        raise ValueError(f"DecodeCompressedCache: interval {interval} must be >= window_size {W}")
    if method == _kvc.PYRAMIDKV:
        return method, cluster._budget(2 * cluster.max_capacity_prompt) + W, W
    return method, cluster.max_capacity_prompt, W


def decode_trigger(P, T, B, W, interval):
    """The one statement of the trigger: a layer holding P prefix rows and T decoded rows after a step compresses now."""
    return P + T >= B + interval and T >= W


class DecodeCompressedLayer(CompressedDynamicLayer):
    """A CompressedDynamicLayer whose decoded rows are compressed again, so that the layer stays bounded during long generations.

    Budget B (fixed per layer and prompt, from the prefill's knobs): SnapKV / StreamingLLM max_capacity_prompt; PyramidKV
    cluster._budget(2 * max_capacity_prompt) + W, the layer's pyramid budget for a prompt long enough to take the per-layer branch.
    After every decode step (attention included) the layer holds S = P + T rows, P per query head (the prefix) and T decoded rows
    since the last compression.  When S >= B + interval and T >= W, the S rows are replaced by the B rows kvc_compress (dot_mode
    EXACT, the current TIE_MODE) keeps of them, scored by the post-RoPE queries of the last W decoded rows, with k = B - W and
    the cluster's kernel_size / pooling; the step's own attention has already seen all S rows, as a prefill's attention sees
    the whole prompt.  `true_length` keeps counting every token; get_mask_sizes reports the rows really stored.

    SPLIT form (the fused step): kvc_decode_compress reads prefix and tail where they are and writes the B rows into the other
    of two prefix buffers of exactly B rows (the prefill's buffer is dropped at the first compression); the tail buffer is
    reused.  EXPANDED form (update: bsz > 1, beams, output_attentions, DECODE_KERNEL = 0): kvc_compress_batch with dot_mode
    EXACT over the [b, H_q, S, D] buffer into the other buffer.  The queries live in a ring [b, H_q, W, D]: decoded row r at
    slot r % W, written only by steps that end with S > B + interval - W (the only rows a next window can hold); StreamingLLM
    needs none.  Nothing on this path copies from the device to the host: the trigger is host
    arithmetic on the lengths the layer tracks.  KVC_DOT_MODE = mfma16 does not apply here."""

    def __init__(self, interval=128):
        _check_interval(interval)
        super().__init__()
        self.interval = interval
        self._kalt = self._valt = None      # the other prefix buffers [b, H_q, capacity, D]: compressions alternate between the two
        self._clear_decode()

    def _clear_decode(self):
        self._qring = None                  # post-RoPE queries [b, H_q, W, D] of the decoded rows, row r at slot r % W
        self._p0 = self._stored             # rows of the prefix (the rest of an EXPANDED buffer are decoded rows)
        self._plan = None                   # (method, B, W) of this prompt, set at its first decode step
        self.compressions = 0

    _batch_tensors = CompressedDynamicLayer._batch_tensors + ("_kalt", "_valt", "_qring")
    _batched_step = False
    reserve_rows = _uniform_rows_only

    def reset(self):
        super().reset()
        self._kalt = self._valt = None
        self._clear_decode()

    def prefill(self, k_compressed, v_compressed, true_length):
        super().prefill(k_compressed, v_compressed, true_length)
        self._clear_decode()

    def update(self, key_states, value_states, *args, **kwargs):
        if self._kbuf is None:
            raise NotImplementedError("kvcache_factory_amd: DecodeCompressedCache needs a model patched with snapkv, pyramidkv or "
                                      "streamingllm (this layer never went through a compressing prefill, e.g. fullkv)")
        return super().update(key_states, value_states, *args, **kwargs)

    def rows(self):
        """(P, T): prefix rows per query head and decoded rows since the prefill or the last compression."""
        if self._split:
            return self._stored, self._tail
        return self._p0, self._stored - self._p0

    def budget(self, cluster):
        """(method, B, W) of this layer for `cluster` (the patched forward's kv_cluster)."""
        return decode_budget(cluster, self.interval)

    def after_decode(self, cluster, query_states):
        from . import _kvc
        if self._plan is None:
            self._plan = self.budget(cluster)
        method, B, W = self._plan
        P, T = self.rows()
        S, t = P + T, query_states.shape[-2]
        if method != _kvc.STREAMINGLLM and S > B + self.interval - W:
            self._ring_write(query_states, S - t, W)
        if decode_trigger(P, T, B, W, self.interval):
            self._compress(cluster, method, B, W, P, T)

    def _ring_write(self, q, r0, W):
        """Query rows r0 .. r0 + t - 1 of this step into slots r % W (only the last W of them can matter)."""
        b, h, t, d = q.shape
        if self._qring is None or self._qring.shape != (b, h, W, d) or self._qring.dtype != q.dtype:
            self._qring = torch.empty(b, h, W, d, dtype=q.dtype, device=q.device)
        m = min(t, W)
        r0, q = r0 + t - m, q[:, :, t - m:]
        s0 = r0 % W
        n1 = min(m, W - s0)
        self._qring[:, :, s0:s0 + n1].copy_(q[:, :, :n1])
        if m > n1:
            self._qring[:, :, :m - n1].copy_(q[:, :, n1:])

    def _fits(self, t, rows):
        """t is a whole allocation of exactly [b, H_q, rows, D] in the cache's dtype: it may serve as an alternate prefix buffer."""
        kb = self._kbuf
        return t is not None and t.shape == (kb.shape[0], kb.shape[1], rows, kb.shape[3]) and t.dtype == kb.dtype and \
            t.device == kb.device and t.untyped_storage().nbytes() == t.numel() * t.element_size()

    def _alt(self, rows):
        """The other prefix buffers: exactly `rows` rows per head (B in the SPLIT form, B + interval + RESERVE in the EXPANDED one)."""
        if not (self._fits(self._kalt, rows) and self._fits(self._valt, rows)):
            kb = self._kbuf
            self._kalt = self._valt = None                                # (released before the new pair is allocated)
            self._kalt = torch.empty(kb.shape[0], kb.shape[1], rows, kb.shape[3], dtype=kb.dtype, device=kb.device)
            self._valt = torch.empty_like(self._kalt)
        return self._kalt, self._valt

    def _compress(self, cluster, method, B, W, P, T):
        from . import _kvc
        from . import pyramidkv_utils as pu
        S, k = P + T, B - W
        scoring = method != _kvc.STREAMINGLLM
        ring_start = S % W
        rows = B if self._split else B + self.interval + self.RESERVE      # the EXPANDED form appends behind the prefix
        if self._split:
            kout, vout = self._alt(rows)
            _kvc.decode_compress(method, self._qring if scoring else None, ring_start, self._kbuf, self._vbuf, P, self._ktail, self._vtail,
                                 T, (kout, vout), W, k, cluster.kernel_size, cluster.pooling, pu.TIE_MODE)
            self._tail = 0
        else:
            kout, vout = self._alt(rows)
            q = None
            if scoring:
                q = self._qring if ring_start == 0 else torch.roll(self._qring, -ring_start, dims=2)   # chronological order
            _kvc.compress_batch(method, [q] if scoring else None, [self._kbuf[:, :, :S]], [self._vbuf[:, :, :S]], W, [k],
                                cluster.kernel_size, cluster.pooling if scoring else None, pu.TIE_MODE,
                                q_rows="window" if scoring else "all", n_q_heads=self._kbuf.shape[1], outs=[(kout, vout)], reuse=True,
                                dot_mode="exact")                 # the rule is EXACT whatever KVC_DOT_MODE says
        old_k, old_v = self._kbuf, self._vbuf
        self._kbuf, self._vbuf = kout, vout
        # the buffers compressed from become the next alternate only if they have exactly the size this form needs; the
        # prefill's (spare rows, or a view into a slab shared by a group of layers) is dropped here
        keep = self._fits(old_k, rows) and self._fits(old_v, rows)
        self._kalt, self._valt = (old_k, old_v) if keep else (None, None)
        self._stored = self._p0 = self._pmax = B
        self.compressions += 1


class DecodeCompressedCache(Cache):
    """A transformers Cache of DecodeCompressedLayer, one per hidden layer: the prompt is compressed at prefill as usual, and
    every `interval` decoded tokens each layer is compressed again to its budget, so that memory and per-step attention stay
    bounded during long generations (the reference's README TODO "Support KV cache compression at decoding stage").

        model.generate(ids, past_key_values=DecodeCompressedCache(model.config, interval=128))

    Works with the snapkv, pyramidkv and streamingllm patches; the rule is DecodeCompressedLayer's.  Other methods, merge="pivot"
    and an unpatched model (fullkv) refuse it with NotImplementedError.  interval must be >= the config's window_size."""

    def __init__(self, config, interval=128):
        _check_interval(interval)
        text = config.get_text_config() if hasattr(config, "get_text_config") else config
        self.interval = interval
        super().__init__(layers=[DecodeCompressedLayer(interval) for _ in range(text.num_hidden_layers)])


def bounded_tail_rows(P0, B, interval):
    """Rows the fixed tail of a BoundedDeviceLayer needs with one-token steps: the layer compresses at the first step after which
    P + T >= B + interval and T >= W (decode_trigger; interval >= W).  From the prefill's P0 rows that is T = B + interval - P0
    (or W <= interval when the prefill kept more than that); from then on P = B and it is T = interval."""
    return max(interval, B + interval - P0)


class _FixedBuffersLayer(CompressedDynamicLayer):
    """What the two bounded layers of graph-replayed decoding share: they are made from a prefilled layer (`adopt`), keep every
    buffer for the whole generation and decode through the fused step only, one sequence, one token a step."""

    def prefill(self, *a, **kw):
        raise NotImplementedError(f"kvcache_factory_amd: a {type(self).__name__} is made from a prefilled layer "
                                  f"({type(self).__name__}.adopt)")

    def enter_device_length(self, *a, **kw):
        raise NotImplementedError(f"kvcache_factory_amd: {type(self).__name__} is in its own device-length mode from the start")

    def grow_tail(self):
        raise NotImplementedError(f"kvcache_factory_amd: the tail of a {type(self).__name__} never grows")

    def _fixed(self, *a, **kw):
        raise NotImplementedError(f"kvcache_factory_amd: a {type(self).__name__} keeps fixed buffers for one sequence and decodes "
                                  "through the fused step only (no reference-shaped update, no batch reordering)")

    update = _map_batch = _fixed

    def rows(self):
        """(P, T) of the host mirror."""
        return self._stored, self._tail

    def _one_token(self, key_states):
        b, _, t, _ = key_states.shape
        cap = self._ktail.shape[2]
        if b != 1 or t != 1:
            raise NotImplementedError(f"kvcache_factory_amd: a {type(self).__name__} takes one-token steps of one sequence, got {b} x {t}")
        if self._tail + t > cap:
            raise RuntimeError(f"kvcache_factory_amd: the fixed tail holds {self._tail} of {cap} rows: the owner did not call "
                               f"{self._after_step}() after the last step")


class BoundedDeviceLayer(_FixedBuffersLayer):
    """Decode-stage compression in DEVICE-LENGTH MODE (graph_decode.GraphDecoder(model, interval=N)): DecodeCompressedLayer's budget
    and trigger (decode_budget, decode_trigger) on a layer whose every address is fixed for the whole generation, so that ONE captured
    step replays however long it runs.  One sequence (bsz = 1), one-token steps.

    The K / V prefix buffers hold Pcap = max(P0, B) rows per query head (the prefill's P0 rows are copied in); how many of them are
    in use is a device int32 (`_plen`) the step reads as its per-row prefix length.  The tail holds bounded_tail_rows(P0, B,
    interval) rows and its length lives in this layer's own device counter (PyramidKV layers compress on different steps).  The
    step (kvc_decode_step_dev_ring) also records its query in the W-slot ring, row T at slot T % W; StreamingLLM keeps no ring and
    takes kvc_decode_step_dev.  The step's workspace and the two B-row output buffers of a compression are allocated on entry.

    `_stored` / `_tail` / `true_length` are the host MIRROR, advanced by the owner (`advance`), who then calls `maybe_compress`:
    when the mirror says so, kvc_decode_compress runs eagerly on the step's stream over (P, T) with ring_start = T % W into the
    output buffers, a device copy moves the B rows back into the fixed prefix buffers, and the prefix-length word (B) and the
    counter (0) are set by device ops.  Nothing is read from the device.  `after_decode` does nothing here."""

    def __init__(self, interval=128):
        _check_interval(interval)
        super().__init__()
        self.interval = interval
        self._clear_bounded()

    def _clear_bounded(self):
        self._plen = None                   # int32 [1] on the device: prefix rows in use (the step's prefix_rows_b)
        self._qring = None                  # [1, H_q, W, D]: the query of tail row T at slot T % W (None: StreamingLLM)
        self._kout = self._vout = None      # [1, H_q, B, D]: where a compression writes before the rows are copied back
        self._plan = None                   # (method, B, W)
        self._cluster = None
        self.compressions = 0

    def reset(self):
        super().reset()
        self._clear_bounded()

    _after_step = "maybe_compress"

    @classmethod
    def adopt(cls, layer, cluster, interval, counter, n_kv_heads):
        """The bounded layer that takes over from `layer`, a plain CompressedDynamicLayer right after its prefill (its P0 rows are
        copied).  counter: int32 [1] on the layer's device, this layer's own; it is set to 0 here by a device op."""
        if type(layer) is not CompressedDynamicLayer or layer._kbuf is None:
            raise NotImplementedError(f"kvcache_factory_amd: BoundedDeviceLayer adopts a prefilled CompressedDynamicLayer, not a "
                                      f"{type(layer).__name__}")
        if layer._split or layer._stored != layer._pmax or layer._devlen:
            raise NotImplementedError("kvcache_factory_amd: this layer already holds decoded rows; enter the bounded mode right after "
                                      "the prefill")
        b, hq, _, d = layer._kbuf.shape
        if b != 1 or layer._padded:
            raise NotImplementedError(f"kvcache_factory_amd: decode-stage compression holds one sequence (bsz = 1), got a batch of {b}")
        self = cls(interval)
        method, B, W = self._plan = decode_budget(cluster, interval)
        assert counter.dtype == torch.int32 and counter.numel() == 1 and counter.device == layer._kbuf.device
        from . import _kvc
        P0, dt, dev = layer._stored, layer._kbuf.dtype, layer._kbuf.device
        self.dtype, self.device, self.is_initialized = layer.dtype, layer.device, True
        self.true_length = layer.true_length
        self._kbuf = torch.empty(1, hq, max(P0, B), d, dtype=dt, device=dev)
        self._vbuf = torch.empty_like(self._kbuf)
        self._kbuf[:, :, :P0].copy_(layer._kbuf[:, :, :P0])
        self._vbuf[:, :, :P0].copy_(layer._vbuf[:, :, :P0])
        self._stored = self._pmax = P0
        self._ktail = torch.empty(1, n_kv_heads, bounded_tail_rows(P0, B, interval), d, dtype=dt, device=dev)
        self._vtail = torch.empty_like(self._ktail)
        self._split, self._tail = True, 0
        self._plen = torch.full((1,), P0, dtype=torch.int32, device=dev)
        if method != _kvc.STREAMINGLLM:
            self._qring = torch.empty(1, hq, W, d, dtype=dt, device=dev)
        self._kout = torch.empty(1, hq, B, d, dtype=dt, device=dev)
        self._vout = torch.empty_like(self._kout)
        self._cluster = cluster
        self._devlen, self._dev_counter, self._dev_hold = True, counter, True
        counter.zero_()
        return self

    def _decode_attend_dev(self, query_states, key_states, value_states, scaling):
        from . import _kvc
        self._one_token(key_states)
        t = key_states.shape[2]
        pcap = self._kbuf.shape[2]
        key = (query_states.stride(), key_states.stride())
        if self._dev_ws_key != key:
            nbytes = _kvc.decode_dev_plan(query_states, key_states, self._kbuf, pcap, self._ktail)[1]
            self._dev_ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self._ktail.device)
            self._dev_ws_key = key
        if self._qring is None:
            out = _kvc.decode_step_dev(query_states, key_states, value_states, self._kbuf, self._vbuf, pcap, self._ktail, self._vtail,
                                       self._dev_counter, scaling, rows_b=self._plen, ws=self._dev_ws)
        else:
            out = _kvc.decode_step_dev_ring(query_states, key_states, value_states, self._kbuf, self._vbuf, pcap, self._ktail,
                                            self._vtail, self._dev_counter, scaling, self._qring, rows_b=self._plen, ws=self._dev_ws)
        if not self._dev_hold:
            self.advance(t)
        return out

    def maybe_compress(self):
        """The trigger, from the host mirror, after the owner advanced it for a step.  -> whether the layer compressed."""
        from . import _kvc
        from . import pyramidkv_utils as pu
        method, B, W = self._plan
        P, T = self._stored, self._tail
        if not decode_trigger(P, T, B, W, self.interval):
            return False
        cl = self._cluster
        _kvc.decode_compress(method, self._qring, T % W, self._kbuf, self._vbuf, P, self._ktail, self._vtail, T,
                             (self._kout, self._vout), W, B - W, cl.kernel_size, cl.pooling, pu.TIE_MODE)
        self._kbuf[:, :, :B].copy_(self._kout)
        self._vbuf[:, :, :B].copy_(self._vout)
        self._plen.fill_(B)
        self._dev_counter.zero_()
        self._stored = self._pmax = B
        self._tail = 0
        self.compressions += 1
        return True


def heavy_hitter_budget(cluster, interval):
    """(B, W) of a layer evicted by H2O's rule for `cluster` (the patched forward's kv_cluster): the one statement of the budget rule,
    shared by HeavyHitterLayer and BoundedHeavyHitterLayer."""
    from . import _kvc
    if getattr(cluster, "_method", None) != _kvc.H2O or getattr(cluster, "merge", None) is not None:
        raise NotImplementedError(f"kvcache_factory_amd: HeavyHitterCache is H2O's decode-time rule; it has none for "
                                  f"{type(cluster).__name__} (merge={getattr(cluster, 'merge', None)!r})")
    W = cluster.window_size
    if interval < W:
        raise ValueError(f"HeavyHitterCache: interval {interval} must be >= window_size {W}")
    return cluster.max_capacity_prompt, W


class HeavyHitterLayer(CompressedDynamicLayer):
    """A CompressedDynamicLayer that keeps evicting while it decodes, by H2O's own rule: every stored row carries, per QUERY
    head, the fp32 sum of the attention every later query paid to it, and the rows with the smallest sums go.

    Scores.  Prefill: the prompt is compressed by the H2O path unchanged; kept row j < k starts at the prompt's column sum
    kvc_compress returned for it (widened exactly), the W window rows and every row of a pass-through prompt at 0.  Every
    decode step (kvc_decode_step_scored): for each new token in ascending order and each row visible to it, its own included,
    score += the softmax probability the step's attention used; a row appended by the step starts from 0.

    Eviction.  B = max_capacity_prompt, W = window_size.  After a step (attention and scoring included) the layer holds
    S = P + T rows, P per query head (the prefix) and T decoded rows (the tail, K / V once per KV head, scores per query head).
    When S >= B + interval and T >= W, kvc_decode_evict keeps k = B - W rows by topk(score[0 : S - W], k) under the current
    TIE_MODE, in top-k order, then the last W rows — K, V and scores — in the other of two B-row prefix buffers (each with its
    score buffer); the tail buffers are reused.  `true_length` keeps counting every token.  At most B + interval + t - 1 rows
    are stored per layer, t the tokens of a step.

    SPLIT form only: the scores are a by-product of the fused step, so a step that cannot take it (`update`: bsz > 1, beams,
    output_attentions, DECODE_KERNEL = 0, a sliding window, CPU tensors) is refused instead of silently dropping them.
    Nothing on the decode path copies from the device to the host: the trigger is host arithmetic on the lengths."""

    def __init__(self, interval=128):
        _check_interval(interval)
        super().__init__()
        self.interval = interval
        self._clear_scores()

    def _clear_scores(self):
        self._sbuf = None                   # fp32 [b, H_q, rows of _kbuf]: scores of the prefix rows
        self._stail = None                  # fp32 [b, H_q, rows of _ktail]: scores of the tail rows, one per QUERY head
        self._kalt = self._valt = self._salt = None     # the other prefix buffers: evictions alternate between the two
        self._plan = None                   # (B, W) of this prompt, set at its first decode step
        self.evictions = 0

    _batch_tensors = CompressedDynamicLayer._batch_tensors + ("_sbuf", "_stail", "_kalt", "_valt", "_salt")
    _batched_step = False

    def _one_sequence(self, *a, **kw):
        raise NotImplementedError("kvcache_factory_amd: HeavyHitterCache holds one sequence (bsz = 1): beam search, "
                                  "num_return_sequences > 1 and batches are not supported")
    reserve_rows = reorder_cache = batch_repeat_interleave = batch_select_indices = _one_sequence

    def reset(self):
        super().reset()
        self._clear_scores()

    def prefill(self, k_compressed, v_compressed, true_length):
        if k_compressed.shape[0] != 1:
            self._one_sequence()
        super().prefill(k_compressed, v_compressed, true_length)
        self._clear_scores()
        kb = self._kbuf
        self._sbuf = torch.zeros(kb.shape[0], kb.shape[1], kb.shape[2], dtype=torch.float32, device=kb.device)

    def prefill_scores(self, idx, scores):
        """The H2O compression's own outputs: idx [b, H_q, k] int64 and the prompt's column sums scores [b, H_q, L - W] in the
        cache dtype.  Kept row j starts at float(scores[h][idx[h][j]]); the window rows stay at 0."""
        k = idx.shape[2]
        assert k <= self._stored and idx.shape[:2] == self._sbuf.shape[:2]
        self._sbuf[:, :, :k].copy_(scores.gather(2, idx).to(torch.float32))

    def update(self, key_states, value_states, *args, **kwargs):
        if self._kbuf is None:
            raise NotImplementedError("kvcache_factory_amd: HeavyHitterCache needs a model patched with h2o (this layer never went "
                                      "through a compressing prefill, e.g. fullkv)")
        raise NotImplementedError("kvcache_factory_amd: HeavyHitterCache scores its rows inside the fused decode step; this step "
                                  "cannot take it (bsz > 1 or beams, output_attentions, KVC_DECODE_KERNEL=0, a sliding window, "
                                  "training mode or tensors that are not on the GPU) and is refused rather than left unscored")

    def rows(self):
        """(P, T): prefix rows per query head and decoded rows since the prefill or the last eviction."""
        return self._stored, (self._tail if self._split else 0)

    def scores(self):
        """fp32 [b, H_q, P + T]: the score of every stored row, prefix then tail (a copy; tests and tools)."""
        P, T = self.rows()
        if self._sbuf is None:
            return None
        pre = self._sbuf[:, :, :P]
        return pre.clone() if T == 0 else torch.cat([pre, self._stail[:, :, :T]], dim=2)

    def budget(self, cluster):
        """(B, W) of this layer for `cluster` (the patched forward's kv_cluster)."""
        return heavy_hitter_budget(cluster, self.interval)

    def decode_attend(self, query_states, key_states, value_states, scaling):
        """One decode step in the SPLIT form (kvc_decode_step_scored): the step's rows [1, H_kv, t, D] go to the tail, every
        visible row's score grows by the attention it received, and the attention output [1, t, H_q, D] comes back."""
        from . import _kvc
        b, hkv, t, d = key_states.shape
        if b != 1:
            self._one_sequence()
        hq = self._kbuf.shape[1]
        if not self._split:
            self._split, self._tail = True, 0
        if self._ktail is None:
            self._ktail = torch.empty(b, hkv, max(self.RESERVE, t), d, dtype=key_states.dtype, device=key_states.device)
            self._vtail = torch.empty_like(self._ktail)
            self._stail = torch.empty(b, hq, self._ktail.shape[2], dtype=torch.float32, device=key_states.device)
        if self._tail + t > self._ktail.shape[2]:                 # tail full: double it (K, V and scores)
            cap, n = max(2 * self._ktail.shape[2], self._tail + t), self._tail
            kt = torch.empty(b, hkv, cap, d, dtype=self._ktail.dtype, device=self._ktail.device)
            vt = torch.empty_like(kt)
            st = torch.empty(b, hq, cap, dtype=torch.float32, device=self._ktail.device)
            kt[:, :, :n].copy_(self._ktail[:, :, :n])
            vt[:, :, :n].copy_(self._vtail[:, :, :n])
            st[:, :, :n].copy_(self._stail[:, :, :n])
            self._ktail, self._vtail, self._stail = kt, vt, st
        out = _kvc.decode_step_scored(query_states, key_states, value_states, self._kbuf, self._vbuf, self._stored,
                                      self._ktail, self._vtail, self._tail, self._sbuf, self._stail, scaling)
        self._tail += t
        self.true_length += t
        return out

    def after_decode(self, cluster, query_states):
        if self._plan is None:
            self._plan = self.budget(cluster)
        B, W = self._plan
        P, T = self.rows()
        if P + T >= B + self.interval and T >= W:
            self._evict(B, W, P, T)

    def _fits(self, t, shape, dtype):
        """t is a whole allocation of exactly `shape`: it may serve as an alternate prefix (or score) buffer."""
        return t is not None and tuple(t.shape) == shape and t.dtype == dtype and t.device == self._kbuf.device and \
            t.untyped_storage().nbytes() == t.numel() * t.element_size()

    def _alt(self, rows):
        """The other prefix buffers and their score buffer: exactly `rows` rows per head."""
        kb = self._kbuf
        kshape, sshape = (kb.shape[0], kb.shape[1], rows, kb.shape[3]), (kb.shape[0], kb.shape[1], rows)
        if not (self._fits(self._kalt, kshape, kb.dtype) and self._fits(self._valt, kshape, kb.dtype) and
                self._fits(self._salt, sshape, torch.float32)):
            self._kalt = self._valt = self._salt = None                   # (released before the new set is allocated)
            self._kalt = torch.empty(kshape, dtype=kb.dtype, device=kb.device)
            self._valt = torch.empty_like(self._kalt)
            self._salt = torch.empty(sshape, dtype=torch.float32, device=kb.device)
        return self._kalt, self._valt, self._salt

    def _evict(self, B, W, P, T):
        from . import _kvc
        from . import pyramidkv_utils as pu
        kout, vout, sout = self._alt(B)
        _kvc.decode_evict(self._kbuf, self._vbuf, P, self._ktail, self._vtail, T, self._sbuf, self._stail, (kout, vout), sout,
                          W, B - W, pu.TIE_MODE)
        old = (self._kbuf, self._vbuf, self._sbuf)
        self._kbuf, self._vbuf, self._sbuf = kout, vout, sout
        # the buffers evicted from become the next alternates only if they have exactly B rows; a prefill's buffer with spare
        # rows (a pass-through prompt) is dropped here
        kshape = tuple(kout.shape)
        keep = self._fits(old[0], kshape, kout.dtype) and self._fits(old[1], kshape, kout.dtype) and \
            self._fits(old[2], kshape[:3], torch.float32)
        self._kalt, self._valt, self._salt = old if keep else (None, None, None)
        self._tail = 0
        self._stored = self._pmax = B
        self.evictions += 1


class HeavyHitterCache(Cache):
    """A transformers Cache of HeavyHitterLayer, one per hidden layer: H2O as its paper runs it — the prompt is compressed at
    prefill by the h2o patch as usual, every decode step adds the attention each cached row received to the row's score inside
    the fused step, and every `interval` decoded tokens each layer drops its lowest-scoring rows back to max_capacity_prompt, so
    memory and per-step attention stay bounded during long generations.

        monkeypatch.replace_llama("h2o")
        model.generate(ids, past_key_values=HeavyHitterCache(model.config, interval=128))

    Works with the h2o patch only, bsz = 1; other methods, merge="pivot", an unpatched model (fullkv), batches / beams and steps
    the fused decode kernel cannot take refuse it with NotImplementedError.  interval must be >= the config's window_size."""

    def __init__(self, config, interval=128):
        _check_interval(interval)
        text = config.get_text_config() if hasattr(config, "get_text_config") else config
        self.interval = interval
        super().__init__(layers=[HeavyHitterLayer(interval) for _ in range(text.num_hidden_layers)])


class BoundedHeavyHitterLayer(_FixedBuffersLayer):
    """H2O's eviction in DEVICE-LENGTH MODE (graph_decode.GraphDecoder(model, heavy_hitter=N)): HeavyHitterLayer's scores, budget and
    trigger (heavy_hitter_budget, decode_trigger) on a layer whose every address is fixed for the whole generation, so that ONE
    captured step replays however long it runs.  BoundedDeviceLayer's twin: one sequence (bsz = 1), one-token steps.

    The K / V prefix buffers and the fp32 score prefix buffer hold Pcap = max(P0, B) rows per query head (the prefill's P0 rows and
    their scores — the prompt's column sums, or zeros for a pass-through prompt — are copied in); how many are in use is a device int32
    (`_plen`) the step reads as its per-row prefix length.  The tail holds bounded_tail_rows(P0, B, interval) rows — K / V per KV head,
    scores [1, H_q, cap] per query head — and its length lives in this layer's own device counter.  The step is
    kvc_decode_step_dev_scored; its workspace and the B-row output buffers of an eviction (K, V, scores) are allocated on entry.

    `_stored` / `_tail` / `true_length` are the host MIRROR, advanced by the owner (`advance`), who then calls `maybe_evict`: when the
    mirror says so, kvc_decode_evict runs eagerly on the step's stream over (P, T) under pyramidkv_utils.TIE_MODE into the output
    buffers, device copies move the B rows of K, V and scores back into the fixed prefix buffers, and the prefix-length word (B) and
    the counter (0) are set by device ops.  Nothing is read from the device.  `after_decode` does nothing here."""

    _after_step = "maybe_evict"

    def __init__(self, interval=128):
        _check_interval(interval)
        super().__init__()
        self.interval = interval
        self._clear_bounded()

    def _clear_bounded(self):
        self._plen = None                   # int32 [1] on the device: prefix rows in use (the step's prefix_rows_b)
        self._sbuf = self._stail = None     # fp32 [1, H_q, Pcap] / [1, H_q, cap]: the scores of the prefix and the tail rows
        self._kout = self._vout = self._sout = None     # [1, H_q, B(, D)]: where an eviction writes before the rows are copied back
        self._plan = None                   # (B, W)
        self.evictions = 0

    def reset(self):
        super().reset()
        self._clear_bounded()

    @classmethod
    def adopt(cls, layer, cluster, interval, counter, n_kv_heads):
        """The bounded layer that takes over from `layer`, a HeavyHitterLayer right after its prefill (its P0 rows and their scores
        are copied).  counter: int32 [1] on the layer's device, this layer's own; it is set to 0 here by a device op."""
        if type(layer) is not HeavyHitterLayer or layer._kbuf is None:
            raise NotImplementedError(f"kvcache_factory_amd: BoundedHeavyHitterLayer adopts a prefilled HeavyHitterLayer, not a "
                                      f"{type(layer).__name__}")
        if layer._split or layer._stored != layer._pmax or layer.evictions:
            raise NotImplementedError("kvcache_factory_amd: this layer already holds decoded rows; enter the bounded mode right after "
                                      "the prefill")
        b, hq, _, d = layer._kbuf.shape
        if b != 1:
            raise NotImplementedError(f"kvcache_factory_amd: H2O's decode-time eviction holds one sequence (bsz = 1), got a batch of {b}")
        self = cls(interval)
        B, W = self._plan = heavy_hitter_budget(cluster, interval)
        assert counter.dtype == torch.int32 and counter.numel() == 1 and counter.device == layer._kbuf.device
        from . import _kvc
        P0, dt, dev = layer._stored, layer._kbuf.dtype, layer._kbuf.device
        pcap, cap = max(P0, B), bounded_tail_rows(P0, B, interval)
        self.dtype, self.device, self.is_initialized = layer.dtype, layer.device, True
        self.true_length = layer.true_length
        self._kbuf = torch.empty(1, hq, pcap, d, dtype=dt, device=dev)
        self._vbuf = torch.empty_like(self._kbuf)
        self._sbuf = torch.empty(1, hq, pcap, dtype=torch.float32, device=dev)
        self._kbuf[:, :, :P0].copy_(layer._kbuf[:, :, :P0])
        self._vbuf[:, :, :P0].copy_(layer._vbuf[:, :, :P0])
        self._sbuf[:, :, :P0].copy_(layer._sbuf[:, :, :P0])
        self._stored = self._pmax = P0
        self._ktail = torch.empty(1, n_kv_heads, cap, d, dtype=dt, device=dev)
        self._vtail = torch.empty_like(self._ktail)
        self._stail = torch.empty(1, hq, cap, dtype=torch.float32, device=dev)
        self._split, self._tail = True, 0
        self._plen = torch.full((1,), P0, dtype=torch.int32, device=dev)
        self._kout = torch.empty(1, hq, B, d, dtype=dt, device=dev)
        self._vout = torch.empty_like(self._kout)
        self._sout = torch.empty(1, hq, B, dtype=torch.float32, device=dev)
        # the step's own workspace: its size follows the bound alone (the strides of a step's q / k_new do not enter it)
        q1, k1 = (torch.empty(1, h, 1, d, dtype=dt, device="meta") for h in (hq, n_kv_heads))
        nbytes = _kvc.decode_dev_scored_plan(q1, k1, self._kbuf, pcap, self._ktail, self._sbuf, self._stail)[1]
        self._dev_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._devlen, self._dev_counter, self._dev_hold = True, counter, True
        counter.zero_()
        return self

    def scores(self):
        """fp32 [1, H_q, P + T]: the score of every stored row of the mirror, prefix then tail (a copy; tests and tools)."""
        P, T = self.rows()
        if self._sbuf is None:
            return None
        return torch.cat([self._sbuf[:, :, :P], self._stail[:, :, :T]], dim=2)

    def scores_state(self):
        """Copies of the two score buffers (device ops): what `set_scores_state` puts back.  For an owner whose warm-up steps before a
        capture must leave no trace — a step rewrites its own K / V row, but what it added to the scores stays."""
        return self._sbuf.clone(), self._stail.clone()

    def set_scores_state(self, state):
        self._sbuf.copy_(state[0])
        self._stail.copy_(state[1])

    def _decode_attend_dev(self, query_states, key_states, value_states, scaling):
        from . import _kvc
        self._one_token(key_states)
        out = _kvc.decode_step_dev_scored(query_states, key_states, value_states, self._kbuf, self._vbuf, self._kbuf.shape[2], self._ktail,
                                          self._vtail, self._dev_counter, self._sbuf, self._stail, scaling, rows_b=self._plen,
                                          ws=self._dev_ws)
        if not self._dev_hold:
            self.advance(key_states.shape[2])
        return out

    def maybe_evict(self):
        """The trigger, from the host mirror, after the owner advanced it for a step.  -> whether the layer evicted."""
        from . import _kvc
        from . import pyramidkv_utils as pu
        B, W = self._plan
        P, T = self._stored, self._tail
        if not decode_trigger(P, T, B, W, self.interval):
            return False
        _kvc.decode_evict(self._kbuf, self._vbuf, P, self._ktail, self._vtail, T, self._sbuf, self._stail, (self._kout, self._vout),
                          self._sout, W, B - W, pu.TIE_MODE)
        self._kbuf[:, :, :B].copy_(self._kout)
        self._vbuf[:, :, :B].copy_(self._vout)
        self._sbuf[:, :, :B].copy_(self._sout)
        self._plen.fill_(B)
        self._dev_counter.zero_()
        self._stored = self._pmax = B
        self._tail = 0
        self.evictions += 1
        return True


def _check_quant_args(nbits, q_group_size, residual_length):
    if nbits not in (2, 4, 8):
        raise ValueError(f"nbits must be 2, 4 or 8, got {nbits}")
    if q_group_size not in (32, 64, 128):
        raise ValueError(f"q_group_size must be 32, 64 or 128, got {q_group_size}")
    if residual_length < q_group_size or residual_length % q_group_size:
        raise ValueError(f"residual_length must be a positive multiple of q_group_size ({q_group_size}), got {residual_length}")


class QuantizedCompressedLayer(CompressedDynamicLayer):
    """A compressed layer whose cache is stored quantized (KIVI-style; the reference's `--quant_method kivi --nbits N`, which
    hands generate() transformers' quantized cache).  The rule, the packing and the metadata are those of include/kvc.h: keys
    per channel over groups of G stored rows, values per token over groups of G channels, asymmetric round-to-nearest in fp32.

    Segments:  PREFIX — the compressed prompt (k + W rows per query head), quantized once at the layer's first decode step
    (the grouped prefill flush writes K' / V' on a side stream, so this happens on the current stream after it has settled) —
    the full-precision prompt buffers are dropped then;  QUANTIZED TAIL — decoded rows, append-only: a block, once quantized,
    is never re-quantized;  RESIDUAL — full-precision decoded rows.  After every step, once the residual holds at least
    R = residual_length rows, its oldest floor(rows / G) * G rows are quantized onto the tail and the rest move to the front.

    This departs on purpose from transformers' QuantizedLayer, which de-quantizes and re-quantizes the WHOLE cache every time
    its residual fills: that costs time proportional to the cache and compounds the rounding error.  The reference's own
    quantizers (HQQ's optimiser, quanto's MaxOptimizer) are not reproduced, so its bytes are not claimed.

    Two forms, as in CompressedDynamicLayer, and one per generation (switching raises RuntimeError):  FUSED (`decode_attend`,
    kvc_decode_step_quant) — tail and residual per KV head, one kernel over all four segments;  REFERENCE-SHAPED (`update`,
    taken when the fused step does not apply: bsz > 1 / beams, output_attentions, DECODE_KERNEL = 0) — tail and residual per
    incoming head, returns cat(de-quantized prefix, de-quantized tail, residual + new rows).  A layer that never went through
    `prefill` (fullkv) takes its first `update` as the prefix and returns those inputs unquantized, as transformers does."""

    RES_SPARE = 64                      # residual rows beyond residual_length (the step's new rows land there)

    def __init__(self, nbits=4, q_group_size=64, residual_length=128):
        _check_quant_args(nbits, q_group_size, residual_length)
        super().__init__()
        self.nbits, self.group_size, self.residual_length = nbits, q_group_size, residual_length
        self._clear_quant()

    def _clear_quant(self):
        self._pkc = self._pvc = self._pkm = self._pvm = None     # prefix: codes [b, H, P, D*nbits/8], metadata (kvc.h)
        self._tkc = self._tvc = self._tkm = self._tvm = None     # quantized tail, same layout, capacity rows per head
        self._rk = self._rv = None                               # residual [b, H, capacity, D], full precision
        self._prows = self._trows = self._rrows = 0
        self._mode = None                                        # None, "fused" or "shaped"

    _batch_tensors = CompressedDynamicLayer._batch_tensors + ("_pkc", "_pvc", "_pkm", "_pvm", "_tkc", "_tvc", "_tkm", "_tvm", "_rk", "_rv")
    _batched_step = False
    reserve_rows = _uniform_rows_only

    def reset(self):
        super().reset()
        self._clear_quant()

    def prefill(self, k_compressed, v_compressed, true_length):
        self._clear_quant()
        super().prefill(k_compressed, v_compressed, true_length)

    # ---- segments ------------------------------------------------------------------------------------------------------
    def _seg(self, which):
        if which == "prefix":
            return None if self._pkc is None else (self._pkc, self._pvc, self._pkm, self._pvm, self._prows)
        return None if self._tkc is None else (self._tkc, self._tvc, self._tkm, self._tvm, self._trows)

    def _quantize_into(self, k, v, bufs, row0, seg=None):
        from . import _kvc
        kc, vc, km, vm = bufs
        _kvc.quantize_rows(k, kc, km, row0, _kvc.QUANT_KEYS, self.nbits, self.group_size)
        _kvc.quantize_rows(v, vc, vm, row0, _kvc.QUANT_VALUES, self.nbits, self.group_size)

    def _set_prefix(self, k, v):
        from . import _kvc
        b, h, n, d = k.shape
        bufs = _kvc.quant_buffers(b, h, n, d, self.nbits, self.group_size, k.device)
        self._quantize_into(k, v, bufs, 0, "prefix")
        self._pkc, self._pvc, self._pkm, self._pvm = bufs
        self._prows = n

    def _quantize_prefix(self):
        """The compressed prompt -> the quantized prefix; the full-precision prompt buffers go."""
        if self._pkc is None and self._kbuf is not None:
            self._set_prefix(self._kbuf[:, :, :self._stored], self._vbuf[:, :, :self._stored])
            self._kbuf = self._vbuf = None
            self._stored = 0

    def _ensure_residual(self, like, t):
        b, h, _, d = like.shape
        if self._rk is None:
            self._rk = torch.empty(b, h, self.residual_length + max(self.RES_SPARE, t), d, dtype=like.dtype, device=like.device)
            self._rv = torch.empty_like(self._rk)
        elif self._rrows + t > self._rk.shape[2]:
            rk = torch.empty(b, h, self._rrows + t + self.RES_SPARE, d, dtype=self._rk.dtype, device=self._rk.device)
            rv = torch.empty_like(rk)
            rk[:, :, :self._rrows].copy_(self._rk[:, :, :self._rrows])
            rv[:, :, :self._rrows].copy_(self._rv[:, :, :self._rrows])
            self._rk, self._rv = rk, rv

    def _flush(self):
        """Once the residual holds >= R rows: its oldest floor(rows / G) * G rows onto the quantized tail, the rest to the front."""
        from . import _kvc
        if self._rrows < self.residual_length:
            return
        G = self.group_size
        n = self._rrows // G * G
        b, h, _, d = self._rk.shape
        need = self._trows + n
        if self._tkc is None or need > self._tkc.shape[2]:
            self._grow_tail(need)
        self._quantize_into(self._rk[:, :, :n], self._rv[:, :, :n], (self._tkc, self._tvc, self._tkm, self._tvm), self._trows, "tail")
        rest = self._rrows - n
        if rest:
            self._rk[:, :, :rest] = self._rk[:, :, n:n + rest].clone()
            self._rv[:, :, :rest] = self._rv[:, :, n:n + rest].clone()
        self._trows, self._rrows = need, rest

    def _grow_tail(self, need):
        """Quantized tail capacity for `need` rows: capacity doubles, quantized bytes are copied as they are."""
        from . import _kvc
        G = self.group_size
        b, h, _, d = self._rk.shape
        cap = max(need, 4 * self.residual_length, 0 if self._tkc is None else 2 * self._tkc.shape[2])
        bufs = _kvc.quant_buffers(b, h, cap, d, self.nbits, G, self._rk.device)
        if self._tkc is not None and self._trows:
            for new, old, rows in zip(bufs, (self._tkc, self._tvc, self._tkm, self._tvm),
                                      (self._trows, self._trows, self._trows // G, self._trows)):
                new[:, :, :rows].copy_(old[:, :, :rows])
        self._tkc, self._tvc, self._tkm, self._tvm = bufs

    def _enter(self, mode):
        if self._mode is not None and self._mode != mode:
            raise RuntimeError(f"kvcache_factory_amd: this quantized layer decodes in the {self._mode} form; it cannot switch to the "
                               f"{mode} form in the middle of a generation (bsz, output_attentions and DECODE_KERNEL must stay as they were)")
        self._mode = mode

    # ---- the reference's view ------------------------------------------------------------------------------------------
    def _qview(self, which):
        from . import _kvc
        if self._pkc is None:                                   # prompt not quantized yet: the compressed prompt as it was written
            buf = self._kbuf if which == "k" else self._vbuf
            return None if buf is None else buf[:, :, :self._stored]
        k = which == "k"
        parts = [self._dequant("prefix", k, self._prows)]
        hq = parts[0].shape[1]
        if self._trows:
            t = self._dequant("tail", k, self._trows)
            parts.append(t.repeat_interleave(hq // t.shape[1], dim=1))
        if self._rrows:
            r = (self._rk if k else self._rv)[:, :, :self._rrows]
            parts.append(r.repeat_interleave(hq // r.shape[1], dim=1))
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=2)

    def _dequant(self, seg, k, rows):
        from . import _kvc
        mode = _kvc.QUANT_KEYS if k else _kvc.QUANT_VALUES
        if seg == "prefix":
            codes, meta = (self._pkc, self._pkm) if k else (self._pvc, self._pvm)
        else:
            codes, meta = (self._tkc, self._tkm) if k else (self._tvc, self._tvm)
        return _kvc.dequantize_rows(codes, meta, 0, rows, mode, self.nbits, self.group_size, self.dtype)

    keys = property(lambda self: self._qview("k"), _placeholder_only("keys"))
    values = property(lambda self: self._qview("v"), _placeholder_only("values"))

    # ---- decode: the reference-shaped path -----------------------------------------------------------------------------
    def update(self, key_states, value_states, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        t = key_states.shape[-2]
        if self._pkc is None and self._kbuf is None:            # a layer that never went through prefill(): this is the prefix
            self._set_prefix(key_states, value_states)
            self.true_length += t
            return key_states, value_states
        self._enter("shaped")
        self._quantize_prefix()
        self._ensure_residual(key_states, t)
        self._rk[:, :, self._rrows:self._rrows + t].copy_(key_states)
        self._rv[:, :, self._rrows:self._rrows + t].copy_(value_states)
        self._rrows += t
        self.true_length += t
        k, v = self.keys, self.values
        self._flush()
        return k, v

    # ---- decode: the fused step ----------------------------------------------------------------------------------------
    def decode_attend(self, query_states, key_states, value_states, scaling):
        """One decode step (kvc_decode_step_quant): the step's rows [bsz, H_kv, t, D] go to the residual and the attention output
        [bsz, t, H_q, D] over quantized prefix, quantized tail and residual comes back; then the residual flush rule."""
        from . import _kvc
        self._enter("fused")
        self._quantize_prefix()
        t = key_states.shape[-2]
        self._ensure_residual(key_states, t)
        out = self._decode_step(query_states, key_states, value_states, scaling)
        self._rrows += t
        self.true_length += t
        self._flush()
        return out

    def _decode_step(self, query_states, key_states, value_states, scaling):
        from . import _kvc
        return _kvc.decode_step_quant(query_states, key_states, value_states, self._seg("prefix"), self._seg("tail"), self._rk, self._rv,
                                      self._rrows, scaling, self.nbits, self.group_size, self.residual_length)

    def can_split(self):
        return self._pkc is not None or self._kbuf is not None

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------
    def stored_length(self):
        pre = self._prows if self._pkc is not None else (self._stored if self._kbuf is not None else 0)
        return pre + self._trows + self._rrows


class QuantizedCompressedCache(Cache):
    """A transformers Cache of QuantizedCompressedLayer, one per hidden layer: the compressed prompt and the decoded tokens are
    stored at `nbits` bits (2, 4 or 8), keys grouped per channel and values per token in groups of `q_group_size`, the last
    < residual_length decoded tokens in full precision.  The keyword names are those of transformers' QuantizedCache, so the
    reference's `cache_config` values carry over:

        model.generate(ids, past_key_values=QuantizedCompressedCache(model.config, nbits=2))

    `backend`, `axis_key` and `axis_value` are refused: the grouping here is fixed (KIVI's)."""

    def __init__(self, config, nbits=4, q_group_size=64, residual_length=128, backend=None, axis_key=None, axis_value=None):
        for name, val in (("backend", backend), ("axis_key", axis_key), ("axis_value", axis_value)):
            if val is not None:
                raise ValueError(f"QuantizedCompressedCache: `{name}` is not configurable — keys are quantized per channel and values "
                                 "per token with this library's own HIP kernels (include/kvc.h)")
        _check_quant_args(nbits, q_group_size, residual_length)
        text = config.get_text_config() if hasattr(config, "get_text_config") else config
        self.nbits, self.q_group_size, self.residual_length = nbits, q_group_size, residual_length
        super().__init__(layers=[QuantizedCompressedLayer(nbits, q_group_size, residual_length) for _ in range(text.num_hidden_layers)])


def quant_flush(res_rows, tail_rows, capacity, residual_length):
    """QuantizedCompressedLayer's flush rule for one-token steps on a quantized tail of FIXED capacity, from host integers alone:
    -> (rows that move from the residual onto the tail now, times the tail's capacity must double first).  The residual is flushed
    whole once it holds residual_length rows (a multiple of the group size, so nothing stays behind)."""
    if res_rows < residual_length:
        return 0, 0
    doublings = 0
    while tail_rows + res_rows > capacity:
        capacity, doublings = 2 * capacity, doublings + 1
    return res_rows, doublings


def quant_schedule(residual_length, capacity, steps):
    """What `steps` one-token steps do to a QuantizedDeviceLayer whose tail starts empty with `capacity` rows: -> (the steps (from 1)
    after which the residual is flushed, the tail rows after each flush, the grow events, the captures of a decoder that captures
    before the first step and again before the first step after every grow event).  Host arithmetic only."""
    flushes, tails, grows, captures = [], [], 0, 0
    res = tail = 0
    stale = True
    for step in range(1, steps + 1):
        if stale:
            captures, stale = captures + 1, False
        res += 1
        rows, doublings = quant_flush(res, tail, capacity, residual_length)
        if rows:
            if doublings:
                capacity, grows, stale = capacity << doublings, grows + 1, True
            tail, res = tail + rows, 0
            flushes.append(step)
            tails.append(tail)
    return flushes, tails, grows, captures


class QuantizedDeviceLayer(_FixedBuffersLayer):
    """The quantized (KIVI-style) cache in DEVICE-LENGTH MODE (graph_decode.GraphDecoder(model, nbits=N)): QuantizedCompressedLayer's
    segments and flush rule on buffers that keep their addresses between grow events, so that a captured step replays while rows are
    decoded and quantized.  One sequence (bsz = 1), one-token steps.

    PREFIX — the compressed prompt, quantized eagerly at adoption by the rule of QuantizedCompressedLayer._set_prefix (the
    full-precision prompt buffers are dropped);  QUANTIZED TAIL — a segment of fixed capacity (a multiple of residual_length) whose
    rows in use live in a device int32 (`_tword`);  RESIDUAL — exactly residual_length full-precision rows per KV head whose rows in
    use live in a second device int32 (`_rword`), advanced by the owner's in-graph add.  The step (kvc_decode_step_quant_dev) reads
    both words and has its own workspace and output buffer.

    `_trows` / `_rrows` / `true_length` are the host MIRROR, advanced by the owner (`advance`), who then calls `maybe_flush`: once
    the mirror says the residual holds residual_length rows they are quantized onto the tail eagerly on the step's stream
    (kvc_quantize_rows for keys and for values, row0 from the mirror), then the tail word += rows and the residual word = 0 by device
    ops.  When the tail cannot take them its capacity doubles first (codes and metadata in use are copied as they are) and
    `maybe_flush` says so: graphs captured over the old buffers are stale.  Nothing is read from the device."""

    def __init__(self, nbits=4, q_group_size=64, residual_length=128):
        _check_quant_args(nbits, q_group_size, residual_length)
        super().__init__()
        self.nbits, self.group_size, self.residual_length = nbits, q_group_size, residual_length
        self._clear_quant()

    def _clear_quant(self):
        self._pkc = self._pvc = self._pkm = self._pvm = None     # prefix: codes [1, H_q, P, D*nbits/8], metadata (kvc.h)
        self._tkc = self._tvc = self._tkm = self._tvm = None     # quantized tail [1, H_kv, capacity, ...]
        self._rk = self._rv = None                               # residual [1, H_kv, residual_length, D], full precision
        self._prows = self._trows = self._rrows = 0
        self._tword = self._rword = None                         # int32 [1] each, on the device: tail rows / residual rows in use
        self._out = None                                         # the step's own output buffer
        self.flushes = 0

    def reset(self):
        super().reset()
        self._clear_quant()

    _after_step = "maybe_flush"
    _qview = QuantizedCompressedLayer._qview
    _dequant = QuantizedCompressedLayer._dequant
    keys = property(lambda self: self._qview("k"), _placeholder_only("keys"))
    values = property(lambda self: self._qview("v"), _placeholder_only("values"))

    @classmethod
    def adopt(cls, layer, nbits, q_group_size, residual_length, tail_rows, tail_word, res_word, n_kv_heads):
        """The quantized layer that takes over from `layer`, a plain CompressedDynamicLayer right after its prefill: its rows are
        quantized into the prefix.  tail_rows: the quantized tail's first capacity, a multiple of residual_length.  tail_word /
        res_word: int32 [1] each on the layer's device, this layer's own; both are set to 0 here by device ops."""
        if type(layer) is not CompressedDynamicLayer or layer._kbuf is None:
            raise NotImplementedError(f"kvcache_factory_amd: QuantizedDeviceLayer adopts a prefilled CompressedDynamicLayer, not a "
                                      f"{type(layer).__name__}")
        if layer._split or layer._stored != layer._pmax or layer._devlen:
            raise NotImplementedError("kvcache_factory_amd: this layer already holds decoded rows; enter the quantized mode right after "
                                      "the prefill")
        b, hq, _, d = layer._kbuf.shape
        if b != 1 or layer._padded:
            raise NotImplementedError(f"kvcache_factory_amd: the fused quantized step holds one sequence (bsz = 1), got a batch of {b}")
        self = cls(nbits, q_group_size, residual_length)
        if tail_rows < residual_length or tail_rows % residual_length:
            raise ValueError(f"tail_rows must be a positive multiple of residual_length ({residual_length}), got {tail_rows}")
        for w in (tail_word, res_word):
            assert w.dtype == torch.int32 and w.numel() == 1 and w.device == layer._kbuf.device
        from . import _kvc
        P, dt, dev = layer._stored, layer._kbuf.dtype, layer._kbuf.device
        self.dtype, self.device, self.is_initialized = layer.dtype, layer.device, True
        self.true_length = layer.true_length
        bufs = _kvc.quant_buffers(1, hq, P, d, nbits, q_group_size, dev)
        self._quantize_into(layer._kbuf[:, :, :P], layer._vbuf[:, :, :P], bufs, 0)
        self._pkc, self._pvc, self._pkm, self._pvm = bufs
        self._prows = P
        self._tkc, self._tvc, self._tkm, self._tvm = _kvc.quant_buffers(1, n_kv_heads, tail_rows, d, nbits, q_group_size, dev)
        self._rk = torch.empty(1, n_kv_heads, residual_length, d, dtype=dt, device=dev)
        self._rv = torch.empty_like(self._rk)
        self._tword, self._rword = tail_word, res_word
        tail_word.zero_()
        res_word.zero_()
        self._split, self._devlen, self._dev_hold = True, True, True
        return self

    def _quantize_into(self, k, v, bufs, row0):
        from . import _kvc
        kc, vc, km, vm = bufs
        _kvc.quantize_rows(k, kc, km, row0, _kvc.QUANT_KEYS, self.nbits, self.group_size)
        _kvc.quantize_rows(v, vc, vm, row0, _kvc.QUANT_VALUES, self.nbits, self.group_size)

    # ---- the lengths of the host mirror ----------------------------------------------------------------------------------------
    def rows(self):
        """(P, Tq, Rr) of the host mirror."""
        return self._prows, self._trows, self._rrows

    def tail_capacity(self):
        return 0 if self._tkc is None else self._tkc.shape[2]

    def segments(self):
        """((k_codes, v_codes, k_meta, v_meta, rows) of the prefix, of the quantized tail, (k_res, v_res, rows)): the buffers as they
        are, rows from the mirror."""
        return ((self._pkc, self._pvc, self._pkm, self._pvm, self._prows), (self._tkc, self._tvc, self._tkm, self._tvm, self._trows),
                (self._rk, self._rv, self._rrows))

    def advance(self, t):
        """t rows were appended to the residual by a step whose Python did not count them (a replayed graph): the mirror follows."""
        self._rrows += t
        self.true_length += t

    def can_split(self):
        return self._pkc is not None

    def stored_length(self):
        return self._prows + self._trows + self._rrows

    # ---- the step -----------------------------------------------------------------------------------------------------------------
    def _decode_attend_dev(self, query_states, key_states, value_states, scaling):
        from . import _kvc
        b, _, t, _ = key_states.shape
        if b != 1 or t != 1:
            raise NotImplementedError(f"kvcache_factory_amd: a QuantizedDeviceLayer takes one-token steps of one sequence, got {b} x {t}")
        if self._rrows + t > self.residual_length:
            raise RuntimeError(f"kvcache_factory_amd: the residual holds {self._rrows} of {self.residual_length} rows: the owner did "
                               "not call maybe_flush() after the last step")
        pre, qt = (self._pkc, self._pvc, self._pkm, self._pvm, self._prows), (self._tkc, self._tvc, self._tkm, self._tvm, 0)
        key = (self._tkc.shape[2], query_states.stride(), key_states.stride())
        if self._dev_ws_key != key:                                   # once per capacity: the step's own workspace and output
            nbytes = _kvc.decode_quant_dev_plan(query_states, key_states, pre, qt, self._rk, self.nbits, self.group_size,
                                                self.residual_length)[1]
            self._dev_ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self._rk.device)
            if self._out is None:
                self._out = torch.empty(b, t, query_states.shape[1], query_states.shape[3], dtype=query_states.dtype,
                                        device=self._rk.device)
            self._dev_ws_key = key
        out = _kvc.decode_step_quant_dev(query_states, key_states, value_states, pre, qt, self._rk, self._rv, self._tword, self._rword,
                                         scaling, self.nbits, self.group_size, self.residual_length, ws=self._dev_ws, out=self._out)
        if not self._dev_hold:
            self.advance(t)
        return out

    def _grow(self):
        """A quantized tail of twice the capacity; codes and metadata in use are copied as they are."""
        from . import _kvc
        G = self.group_size
        old = (self._tkc, self._tvc, self._tkm, self._tvm)
        _, h, cap, cb = self._tkc.shape
        bufs = _kvc.quant_buffers(1, h, 2 * cap, cb * 8 // self.nbits, self.nbits, G, self._tkc.device)
        if self._trows:
            for new, was, rows in zip(bufs, old, (self._trows, self._trows, self._trows // G, self._trows)):
                new[:, :, :rows].copy_(was[:, :, :rows])
        self._tkc, self._tvc, self._tkm, self._tvm = bufs
        self._dev_ws = self._dev_ws_key = None

    def maybe_flush(self):
        """The flush rule, from the host mirror, after the owner advanced it for a step.  -> (whether the residual was flushed,
        whether the tail grew — graphs captured before are stale then)."""
        rows, doublings = quant_flush(self._rrows, self._trows, self._tkc.shape[2], self.residual_length)
        if not rows:
            return False, False
        for _ in range(doublings):
            self._grow()
        self._quantize_into(self._rk[:, :, :rows], self._rv[:, :, :rows], (self._tkc, self._tvc, self._tkm, self._tvm), self._trows)
        self._tword.add_(rows)
        self._rword.zero_()
        self._trows, self._rrows = self._trows + rows, 0
        self.flushes += 1
        return True, doublings > 0


class RaggedDynamicLayer(_BatchOps, DynamicLayer):
    """The flattened cache of AdaKV / HeadKV for one layer — counterpart of the reference's DynamicCacheSplitHeadFlatten
    (pyramidkv_utils.py:28-102), whose every decode step allocates a new tensor and re-copies the whole cache with one row
    inserted per head (update_flatten_view, csrc/csrc/cuda_api.cu:12-85).  Here every head's segment has spare rows behind it
    and kvc_ragged_decode_step appends in place; when a segment fills up, the cache is re-laid out once with twice the slack."""

    def __init__(self):
        super().__init__()
        self.true_length = 0
        self.k_flat = self.v_flat = self.seg_off = self.seg_len = None
        self.lens, self.slack, self.appended = [], 0, 0

    keys = property(lambda self: self.k_flat, _placeholder_only("keys"))
    values = property(lambda self: self.v_flat, _placeholder_only("values"))

    def _no_batch(self, *a, **kw):
        # the flattened cache has no batch dimension to reorder (the reference's DynamicCacheSplitHeadFlatten has none either, and
        # its README lists batch inference as unsupported): refuse instead of decoding against un-reordered histories
        raise NotImplementedError("AdaKV / HeadKV keep one flattened cache per layer: beam search / num_return_sequences > 1 are not supported")
    reorder_cache = batch_repeat_interleave = batch_select_indices = _no_batch

    def reset(self):
        self.k_flat = self.v_flat = self.seg_off = self.seg_len = None
        self.lens, self.slack, self.appended, self.true_length = [], 0, 0, 0

    def prefill(self, ragged, true_length):
        if not self.is_initialized:
            self.lazy_initialization(ragged["k_flat"], ragged["v_flat"])
        self.k_flat, self.v_flat = ragged["k_flat"], ragged["v_flat"]
        self.seg_off, self.seg_len = ragged["seg_off"], ragged["seg_len"]
        self.lens, self.slack, self.appended = list(ragged["lens"]), ragged["slack"], 0
        self.true_length = int(true_length)

    def _regrow(self, need):
        slack = max(2 * self.slack, need)
        offs, row = [], 0
        for ln in self.lens:
            offs.append(row)
            row += ln + slack
        new_off = torch.tensor(offs, dtype=torch.int64, device=self.k_flat.device)
        kf = torch.empty(row, self.k_flat.shape[1], dtype=self.k_flat.dtype, device=self.k_flat.device)
        vf = torch.empty_like(kf)
        old = self.seg_off.tolist()
        for h, ln in enumerate(self.lens):
            m = ln + self.appended
            kf[offs[h]:offs[h] + m].copy_(self.k_flat[old[h]:old[h] + m])
            vf[offs[h]:offs[h] + m].copy_(self.v_flat[old[h]:old[h] + m])
        self.k_flat, self.v_flat, self.seg_off, self.slack = kf, vf, new_off, slack

    def decode_attend(self, query_states, key_states, value_states, scaling):
        from . import _kvc
        t = key_states.shape[-2]
        if self.appended + t > self.slack:
            self._regrow(self.appended + t)
        out = _kvc.ragged_decode_step(query_states, key_states, value_states, self.k_flat, self.v_flat, self.seg_off, self.seg_len,
                                      self.appended, scaling, slack=self.slack)
        self.appended += t
        self.true_length += t
        return out

    def segments(self):
        """Per head: (keys, values) views of its rows (prefill + appended) — for tests and tools."""
        offs = self.seg_off.tolist()
        return [(self.k_flat[o:o + ln + self.appended], self.v_flat[o:o + ln + self.appended]) for o, ln in zip(offs, self.lens)]

    def get_seq_length(self):
        return self.true_length

    def get_mask_sizes(self, query_length):
        return max(self.lens or [0]) + self.appended + query_length, 0


class ThinkDynamicLayer(_BatchOps, DynamicLayer):
    """ThinK's cache for one layer — counterpart of the reference's cache_utils_think.DynamicCache (key_cache_pruned, mask,
    key_cache, value_cache; `update_think`, cache_utils_think.py:390-424, llama_model_think.py:167-168): the compressed keys are
    stored WITHOUT their pruned channels except the last `recent_size` rows; decoded tokens join the full-channel rows.  A decode
    step attends over [pruned rows | recent + decoded rows] with the query's kept channels for the first part
    (llama_model_think.py:175-196) — here ONE kvc_decode_step2 call (round 2: two torch matmuls, a cat, a softmax and a matmul):
    the pruned keys are kept once more in the kernel's form (kept channels in ascending order, zero-padded to 16 bytes, with the
    channel list), the recent rows and all values stay where update_think wrote them, and the decoded tokens go to a tail stored
    once per KV head and appended in place, as in CompressedDynamicLayer."""
    RESERVE = 256

    def __init__(self):
        super().__init__()
        self.true_length = 0
        self.key_pruned = None          # [bsz, H, P1, Dk] (the reference's layout) or None (pass-through prompt: nothing pruned)
        self.mask = None                # [bsz, H, D] bool, True = channel kept
        self._kp = self._chan = None    # kernel form: [bsz, H, P1, Dk padded], [bsz, H, Dk padded] int16 (-1 = padding)
        self._kbuf = self._vbuf = None  # recent keys [bsz, H, Pr, D]; ALL values of the compressed prompt [bsz, H, P1 + Pr, D]
        self._ktail = self._vtail = None    # decoded tokens [bsz, H_kv, capacity, D]
        self._tail = 0

    def _expanded(self, buf, tail):
        if buf is None:
            return None
        if tail is None or self._tail == 0:
            return buf
        return torch.cat([buf, tail[:, :, :self._tail].repeat_interleave(buf.shape[1] // tail.shape[1], dim=1)], dim=2)

    # the reference's views: key_cache (full-channel rows: recent + decoded) and value_cache (every row)
    keys = property(lambda self: self._expanded(self._kbuf, self._ktail), _placeholder_only("keys"))
    values = property(lambda self: self._expanded(self._vbuf, self._vtail), _placeholder_only("values"))
    _batch_tensors = ("key_pruned", "mask", "_kp", "_chan", "_kbuf", "_vbuf", "_ktail", "_vtail")

    def reset(self):
        self.key_pruned = self.mask = self._kp = self._chan = self._kbuf = self._vbuf = self._ktail = self._vtail = None
        self._tail = self.true_length = 0

    def prefill_think(self, kv_pruned, kv_recent, mask, values, true_length):
        if not self.is_initialized:
            self.lazy_initialization(kv_recent, values)
        self.key_pruned, self.mask = kv_pruned, mask
        b, h, p1, dk = kv_pruned.shape
        per16 = 16 // kv_pruned.element_size()
        dkp = (dk + per16 - 1) // per16 * per16
        self._kp = torch.nn.functional.pad(kv_pruned, (0, dkp - dk)).contiguous()
        # kept channels in ascending order (the order of key_states[mask], pyramidkv_utils.py:24-25): a stable sort of the mask
        order = torch.sort(mask.to(torch.int8), dim=-1, descending=True, stable=True).indices[..., :dk]
        self._chan = torch.nn.functional.pad(order.to(torch.int16), (0, dkp - dk), value=-1).contiguous()
        self._kbuf, self._vbuf = kv_recent.contiguous(), values.contiguous()
        self._ktail = self._vtail = None
        self._tail = 0
        self.true_length = int(true_length)

    def prefill_plain(self, keys, values, true_length):
        """A prompt shorter than the budget (or a merged one): update_think returned plain (keys, values)."""
        if not self.is_initialized:
            self.lazy_initialization(keys, values)
        self.key_pruned = self.mask = self._kp = self._chan = None
        self._kbuf, self._vbuf = keys.contiguous(), values.contiguous()
        self._ktail = self._vtail = None
        self._tail = 0
        self.true_length = int(true_length)

    def attend(self, query_states, k_new, v_new, scaling):
        """The step's K/V rows [bsz, H_kv, t, D] go to the tail and the attention output [bsz, t, H, D] over pruned rows, recent
        rows and tail comes back — kvc_decode_step2 (llama_model_think.py:170-196)."""
        from . import _kvc
        b, hkv, t, d = k_new.shape
        if self._ktail is None:
            self._ktail = torch.empty(b, hkv, max(self.RESERVE, 2 * t), d, dtype=k_new.dtype, device=k_new.device)
            self._vtail = torch.empty_like(self._ktail)
        if self._tail + t > self._ktail.shape[2]:                 # tail full: double it
            cap = max(2 * self._ktail.shape[2], self._tail + t)
            kt = torch.empty(b, hkv, cap, d, dtype=self._ktail.dtype, device=self._ktail.device)
            vt = torch.empty_like(kt)
            kt[:, :, :self._tail].copy_(self._ktail[:, :, :self._tail])
            vt[:, :, :self._tail].copy_(self._vtail[:, :, :self._tail])
            self._ktail, self._vtail = kt, vt
        p1 = 0 if self._kp is None else self._kp.shape[2]
        out = _kvc.decode_step(query_states, k_new, v_new, self._kbuf, self._vbuf, self._kbuf.shape[2], self._ktail, self._vtail,
                               self._tail, scaling, k_pruned=self._kp, chan=self._chan, pruned_rows=p1)
        self._tail += t
        self.true_length += t
        return out

    def stored_length(self):
        return (0 if self._vbuf is None else self._vbuf.shape[2]) + self._tail

    def get_seq_length(self):
        return self.true_length

    def get_mask_sizes(self, query_length):
        return self.stored_length() + query_length, 0


def _check_threshold(outlier_threshold):
    t = float(outlier_threshold)
    if not (t > 0.0 and t != float("inf")):
        raise ValueError(f"outlier_threshold must be finite and > 0, got {outlier_threshold}")
    return t


_POOL_PARTS = ("chan", "val", "used", "ri")


class KVQuantCompressedLayer(QuantizedCompressedLayer):
    """QuantizedCompressedLayer with exact outliers (KVQuant's dense-and-sparse split; the reference's `--quant_method kvquant`):
    every element with |x| > T' (T' = outlier_threshold rounded to the cache dtype) is zeroed in the quantized (dense) part and kept
    exactly in an outlier POOL, one per segment and per keys / values (include/kvc.h: chan, val, used, rowinfo; all indexed by the
    batch row, so beam reordering permutes them like every other buffer).  De-quantized cache = the KIVI values with the outliers
    written back.  Segments, forms and the residual flush are QuantizedCompressedLayer's.

    Host reads of the device counters `used` all go through `_read_used`:
      PREFIX — the prompt is quantized into a pool of an estimated size (1/32 of its elements) and `used` is read back once (the
               layer's first decode step, or the prompt's `update` for fullkv); an overflow repeats the call into a pool of the
               exact size, a smaller count shrinks the pool to it (capacity: max_b used rounded up to 16, at least 16);
      TAIL   — a flush of n rows adds at most W = n * D * H entries per batch row.  The host keeps an upper bound of used (+W per
               flush).  After every flush max_b used is also copied to pinned host memory without waiting (an event marks its
               arrival); the next flush takes that value as its bound if it has arrived, which it normally has R tokens later.  The
               true value is read (blocking) only when bound + W would pass the pool capacity; the pool then grows (entries copied
               byte for byte) whenever fewer than W entries are left.  New tail pools hold 2W entries."""

    PREFIX_EST = 32                     # the prompt's pool is first sized at 1/PREFIX_EST of its elements

    def __init__(self, nbits=4, q_group_size=64, residual_length=128, outlier_threshold=6.0):
        self.outlier_threshold = _check_threshold(outlier_threshold)
        super().__init__(nbits, q_group_size, residual_length)

    def _clear_quant(self):
        super()._clear_quant()
        for pool in ("_pko", "_pvo", "_tko", "_tvo"):          # prefix / tail pools of keys / values
            self._set_pool(pool, None)
        self._tbound = 0                                      # upper bound of max_b used[b] of the tail pools
        self._note = None                                     # (host copy of max_b used after the last flush, its event)

    _batch_tensors = QuantizedCompressedLayer._batch_tensors + tuple(
        f"{pool}_{part}" for pool in ("_pko", "_pvo", "_tko", "_tvo") for part in _POOL_PARTS)

    def _pool(self, name):
        parts = tuple(getattr(self, f"{name}_{p}") for p in _POOL_PARTS)
        return None if parts[0] is None else parts

    def _set_pool(self, name, pool):
        for p, t in zip(_POOL_PARTS, pool if pool is not None else (None,) * 4):
            setattr(self, f"{name}_{p}", t)

    def _read_used(self, *pools):
        """The one place where the host waits for the device: max over the batch of each pool's `used`."""
        return [int(x) for x in torch.stack([p[2] for p in pools]).amax(dim=1).tolist()]

    def _note_used(self, pools):
        """After a flush: max_b used of the tail pools on its way to the host, without waiting."""
        u = torch.stack([p[2] for p in pools]).amax()
        if u.is_cuda:
            if getattr(self, "_used_host", None) is None:
                self._used_host = torch.empty((), dtype=torch.int32, pin_memory=True)
            self._used_host.copy_(u, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._note = (self._used_host, ev)
        else:
            self._note = (u.clone(), None)

    def _take_note(self):
        """The bound from the last flush's copy of used, if it has arrived (no waiting)."""
        if self._note is not None and (self._note[1] is None or self._note[1].query()):
            self._tbound = int(self._note[0])
            self._note = None

    # ---- quantize --------------------------------------------------------------------------------------------------------
    def _quantize_pools(self, k, v, bufs, row0, pools):
        from . import _kvc
        kc, vc, km, vm = bufs
        _kvc.quantize_rows_outliers(k, kc, km, pools[0], row0, _kvc.QUANT_KEYS, self.nbits, self.group_size, self.outlier_threshold)
        _kvc.quantize_rows_outliers(v, vc, vm, pools[1], row0, _kvc.QUANT_VALUES, self.nbits, self.group_size, self.outlier_threshold)

    @staticmethod
    def _resized(pool, cap):
        """The pool with `cap` entries per batch row: its first min(cap, old) entries copied byte for byte, used and rowinfo kept."""
        chan, val, used, ri = pool
        b, old = chan.shape
        c2 = torch.empty(b, cap, dtype=chan.dtype, device=chan.device)
        v2 = torch.empty(b, cap, dtype=val.dtype, device=val.device)
        n = min(cap, old)
        c2[:, :n].copy_(chan[:, :n])
        v2[:, :n].copy_(val[:, :n])
        return c2, v2, used, ri

    def _quantize_into(self, k, v, bufs, row0, seg=None):
        from . import _kvc
        b, h, n, d = k.shape
        if seg == "prefix":
            est = max(16, -(-(h * n * d) // (16 * self.PREFIX_EST)) * 16)
            pools = [_kvc.outlier_pool(b, h, n, est, k.dtype, k.device) for _ in range(2)]
            self._quantize_pools(k, v, bufs, 0, pools)
            used = self._read_used(*pools)
            if max(used) > est:                                       # overflow: again, into pools of the exact size
                pools = [_kvc.outlier_pool(b, h, n, max(16, -(-u // 16) * 16), k.dtype, k.device) for u in used]
                self._quantize_pools(k, v, bufs, 0, pools)
            else:
                pools = [self._resized(p, max(16, -(-u // 16) * 16)) for p, u in zip(pools, used)]
            self._set_pool("_pko", pools[0])
            self._set_pool("_pvo", pools[1])
            return
        W = n * d * h                                                 # worst case of this flush, per batch row
        pools = [self._pool("_tko"), self._pool("_tvo")]
        cap = pools[0][0].shape[1]
        self._take_note()
        if self._tbound + W > cap:
            self._tbound = max(self._read_used(*pools))
            if self._tbound + W > cap:                                # grow: entries copied byte for byte
                cap = max(2 * cap, self._tbound + 2 * W)
                pools = [self._resized(p, cap) for p in pools]
                self._set_pool("_tko", pools[0])
                self._set_pool("_tvo", pools[1])
        self._quantize_pools(k, v, bufs, row0, pools)
        self._tbound += W
        self._note_used(pools)

    def _grow_tail(self, need):
        from . import _kvc
        old = self._trows
        super()._grow_tail(need)
        b, h, cap, _ = self._tkc.shape
        if self._tko_chan is None:                                    # first flush: pools of two worst-case flushes
            W = (need - old) * self._rk.shape[3] * h
            for name in ("_tko", "_tvo"):
                self._set_pool(name, _kvc.outlier_pool(b, h, cap, 2 * W, self._rk.dtype, self._rk.device))
            self._tbound, self._note = 0, None
            return
        for name in ("_tko", "_tvo"):                                 # rowinfo follows the rows' capacity
            chan, val, used, ri = self._pool(name)
            r2 = torch.empty(b, h, cap, dtype=ri.dtype, device=ri.device)
            r2[:, :, :old].copy_(ri[:, :, :old])
            self._set_pool(name, (chan, val, used, r2))

    # ---- de-quantize / decode ---------------------------------------------------------------------------------------------
    def _dequant(self, seg, k, rows):
        from . import _kvc
        mode = _kvc.QUANT_KEYS if k else _kvc.QUANT_VALUES
        if seg == "prefix":
            codes, meta, pool = (self._pkc, self._pkm, self._pool("_pko")) if k else (self._pvc, self._pvm, self._pool("_pvo"))
        else:
            codes, meta, pool = (self._tkc, self._tkm, self._pool("_tko")) if k else (self._tvc, self._tvm, self._pool("_tvo"))
        return _kvc.dequantize_rows_outliers(codes, meta, pool, 0, rows, mode, self.nbits, self.group_size, self.dtype)

    def _decode_step(self, query_states, key_states, value_states, scaling):
        from . import _kvc
        po = (self._pool("_pko"), self._pool("_pvo")) if self._pkc is not None else None
        to = (self._pool("_tko"), self._pool("_tvo")) if self._trows else None
        return _kvc.decode_step_quant_outliers(query_states, key_states, value_states, self._seg("prefix"), self._seg("tail") if self._trows else None,
                                               po, to, self._rk, self._rv, self._rrows, scaling, self.nbits, self.group_size,
                                               self.residual_length)

    def pool_bytes(self):
        """Bytes held by the outlier pools (chan, val, used, rowinfo of every pool)."""
        return sum(t.numel() * t.element_size() for n in self._batch_tensors if n.startswith(("_pko", "_pvo", "_tko", "_tvo"))
                   for t in (getattr(self, n),) if t is not None)


class KVQuantCompressedCache(QuantizedCompressedCache):
    """QuantizedCompressedCache with exact outliers, one KVQuantCompressedLayer per hidden layer: the counterpart of the reference's
    `--quant_method kvquant` (KVQuantizedCache(cache_config, outlier_threshold=6.0)).  The keyword names are the reference's:

        model.generate(ids, past_key_values=KVQuantCompressedCache(model.config, nbits=2, outlier_threshold=6.0))"""

    def __init__(self, config, nbits=4, q_group_size=64, residual_length=128, outlier_threshold=6.0, backend=None, axis_key=None,
                 axis_value=None):
        super().__init__(config, nbits, q_group_size, residual_length, backend, axis_key, axis_value)
        self.outlier_threshold = _check_threshold(outlier_threshold)
        self.layers = [KVQuantCompressedLayer(nbits, q_group_size, residual_length, self.outlier_threshold) for _ in self.layers]
