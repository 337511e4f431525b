"""TEST-ONLY reference and checker for the six decode-step entries of `_kvc` (decode_step with and without ThinK's pruned segment,
decode_step_rows, decode_step_scored, decode_step_quant, decode_step_quant_outliers, ragged_decode_step).  No GPU needed: a case
is built on the CPU, handed to any callable with the entry's signature (the HIP binding on a device, or a CPU stand-in) and judged
against fp64 attention over the VIRTUAL CACHE — per (batch row, query head) the rows the step's tokens may see, in the kernels'
order: ThinK's pruned rows (kept channels, zeros elsewhere) | prefix rows of the query head | quantized tail of the KV head
(quant_ref / kvquant_ref's restated de-quantization) | full-precision tail or residual of the KV head | the step's own rows, causal.
The ragged cache is a per-head prefix (segment + rows appended so far) and the step's rows.

Family A, needles (row-exact): one visible row r* per (batch row, head, token) has the key alpha * q with alpha = 80 sqrt(D) / |q|^2,
so its logit is 80 nats and, checked here in fp64 for every probe, all other visible rows together weigh <= 2^-40.  Values have
|v| in [1/16, 4], so the expected output is V[r*] bit for bit (within 1 ulp of the dtype over a de-quantized row).  Queries of the
tokens of one step are orthogonal (QR of a random matrix), so one token's needle is an ordinary row to the others.  Calls are
either "own" (probes in the per-query-head segments, every head its own query) or "shared" (probes in the per-KV-head segments,
one query per GQA group; V still differs per KV head); "new" probes every new row from its own token and "decoy" puts a key of
160 nats into new row i + 1, invisible to token i, whose needle sits in a visible row.

Family B, peaked heavy-tailed data (queries of standard deviation 1.5, log-normal per-channel scales, a weak sink row) with the
per-element bound   |got - ref64| <= 1/2 ulp_dtype(max(|ref64|, |got|)) + 4 e_ref sum_j p_j |v_j|   where e_ref is the error of the
plain fp32 torch restatement against fp64 on the same tensors, normalised by sum p |v| (heavy_hitter_ref.one_step_bound's margin
of 4 for the kernel's own summation order and exp2).  Quantized entries: e_ref also covers the shift of ref64 when the
de-quantized K and V move by the one fp32 ulp the de-quantization is allowed (two more fp64 attentions, worst signs)."""
import math

import numpy as np
import torch

import kvquant_ref as KQ
import quant_ref as Q

PREC = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}            # significand bits
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}
NEEDLE_NATS, DECOY_NATS, OFF_WEIGHT = 80.0, 160.0, 2.0 ** -40
ENTRIES = ("step2", "think", "rows", "scored", "quant", "outl", "ragged")
QUANTIZED = ("quant", "outl")
SPARE = 7                                                                     # NaN rows behind every dense buffer
FACTOR = 4.0


class ProbeInputError(RuntimeError):
    """A probe whose inputs do not meet the needle condition: an error in the test's inputs, never a skip."""


def ulp(x, dtype):
    """Spacing of `dtype` at |x| (fp64 arrays), the subnormal spacing below the smallest normal."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** MIN_EXP[dtype])))
    return 2.0 ** (e - (PREC[dtype] - 1))


def _rt(x, dtype):
    return x.to(dtype).float()


def _np64(x):
    return x.detach().cpu().to(torch.float64).numpy()


def attention64(q, K, V, n, scaling):
    """fp64 softmax attention over a virtual cache.  q [b, H, t, D]; K, V [b, H, nmax, D] (rows at or past n[b, h] unused);
    token i of (b, h) sees rows [0, n[b, h] - t + i + 1).  Returns (out [b, H, t, D], p [b, H, t, nmax])."""
    t, nmax = q.shape[2], K.shape[2]
    s = np.einsum("bhtd,bhrd->bhtr", q, K) * scaling
    vis = n[:, :, None] - t + np.arange(t)[None, None, :] + 1                 # [b, H, t]
    s = np.where(np.arange(nmax)[None, None, None, :] < vis[..., None], s, -np.inf)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhtr,bhrd->bhtd", p, np.nan_to_num(V)), p


def split_plan(bsz, hq, t, rows):
    """(splits, rows_per_split) of the kernels' split-KV plan (kvc_decode.hip: decode_splits and launch_decode_step)."""
    heads = bsz * hq * t
    s = max(1, min(-(-1024 // heads), -(-rows // 64), 64))
    if s == 1:
        return 1, rows
    rps = -(-(-(-rows // s)) // 64) * 64
    return -(-rows // rps), rps


# ---- a case: source tensors, needles, the entry's arguments, the virtual cache ------------------------------------------------
class Case:
    """spec keys: entry, dtype, D, hq, hkv, b, t, P (int | per batch row | per head for ragged), T (tail / residual rows),
    P1 / keep (ThinK), Tq / nbits / G / R / thr (quantized), appended / slack (ragged), q_view, v_outliers."""

    def __init__(self, spec, family, seed=0, mode="own", call=0):
        d = dict(b=1, T=0, P1=0, keep=0, Tq=0, nbits=4, G=32, R=128, thr=6.0, appended=0, slack=0, q_view=False, v_outliers=False)
        d.update(spec)
        self.__dict__.update(d)
        assert self.entry in ENTRIES and mode in ("own", "shared", "new", "decoy")
        self.family, self.mode, self.call, self.seed = family, mode, call, seed
        self.grp = self.hq // self.hkv
        self.scaling = self.D ** -0.5
        P = np.asarray(self.P)
        if P.ndim == 1 and self.entry == "ragged":
            P = P[None, :]
        elif P.ndim == 1:
            P = P[:, None]
        self.npre = np.broadcast_to(P, (self.b, self.hq)).astype(np.int64).copy()
        self.Pmax = int(self.npre.max())
        if self.entry == "ragged":
            assert self.b == 1 and self.T == 0 and self.slack >= self.appended + self.t and int(self.npre.min()) > self.appended
        if self.entry in QUANTIZED:
            assert self.Tq % self.G == 0 and self.R % self.G == 0 and 0 <= self.T < self.R
        self.n = self.P1 + self.npre + self.Tq + self.T + self.t              # [b, hq] rows of the virtual cache
        self.probes = []                                                      # (b, h, i, virtual row)
        self._scaled = set()
        self._draw()
        if family == "A":
            self._plant()
        self._finalize()
        self._assemble()

    # -- layout ---------------------------------------------------------------------------------------------------------------
    def segments(self, b, h):
        """[(name, first virtual row, rows)] of (b, h), empty segments left out."""
        out, o = [], 0
        for name, rows in (("pruned", self.P1), ("prefix", int(self.npre[b, h])), ("qtail", self.Tq), ("tail", self.T), ("new", self.t)):
            if rows:
                out.append((name, o, rows))
            o += rows
        return out

    def locate(self, b, h, r):
        for name, o, rows in self.segments(b, h):
            if o <= r < o + rows:
                return name, r - o
        raise IndexError(r)

    def probe_rows(self, b, h, kinds):
        """Virtual rows of (b, h) to probe inside the segments named in `kinds`: every row of a cache of <= 320 rows, else rows with
        r mod 32 in {31, 0}; always the first and last row of every segment.  -> (edges, regular), both sorted."""
        n = int(self.n[b, h])
        edges, regular = set(), []
        for name, o, rows in self.segments(b, h):
            if name in kinds:
                edges.update((o, o + rows - 1))
                regular += [r for r in range(o, o + rows) if n <= 320 or r % 32 in (31, 0)]
        return sorted(edges), sorted(set(regular) - edges)

    # -- random data ----------------------------------------------------------------------------------------------------------
    def _draw(self):
        g = self.g = torch.Generator().manual_seed(self.seed)
        b, hq, hkv, t, D, dt = self.b, self.hq, self.hkv, self.t, self.D, self.dtype

        def keys(heads, rows):
            x = torch.randn(b, heads, rows, D, generator=g)
            if self.family == "B":
                x = x * torch.exp(0.5 * torch.randn(b, heads, 1, D, generator=g))
            return _rt(x, dt)

        def vals(heads, rows):
            if self.family == "B":
                return keys(heads, rows)
            mag = torch.exp2(torch.rand(b, heads, rows, D, generator=g) * 6 - 4)          # |v| in [1/16, 4]
            sign = torch.where(torch.rand(b, heads, rows, D, generator=g) < 0.5, -1.0, 1.0)
            return _rt(mag * sign, dt).clamp(-4, 4)
        self.keepmask = torch.ones(b, hq, D, dtype=torch.bool)
        if self.P1:
            self.keepmask.zero_()
            for bi in range(b):
                for h in range(hq):
                    self.keepmask[bi, h, torch.randperm(D, generator=g)[:self.keep]] = True
        self.pk, self.pv = keys(hq, self.P1), vals(hq, self.P1)
        self.ek, self.ev = keys(hq, self.Pmax + SPARE), vals(hq, self.Pmax + SPARE)
        self.qk, self.qv = keys(hkv, self.Tq), vals(hkv, self.Tq)
        self.tk, self.tv = keys(hkv, self.T), vals(hkv, self.T)
        self.nk, self.nv = keys(hkv, t), vals(hkv, t)
        self.keep_spare = torch.zeros(b, hq, self.Pmax + SPARE, dtype=torch.bool)        # spare prefix rows that stay finite (decoys)
        if self.family == "B":
            q = 1.5 * torch.randn(b, hq, t, D, generator=g)
            self.q = _rt(q, dt)
            for bi in range(b):                                                          # a weak sink: 2 nats for the head's first token
                for h in range(hq):
                    qs = self.q[bi, h, 0].double() * self.keepmask[bi, h]
                    vec = (2.0 * math.sqrt(D) / float(qs @ qs)) * qs
                    if self.P1:
                        self.pk[bi, h, 0] = _rt(vec.float(), dt)
                    elif self.npre[bi, h]:
                        self.ek[bi, h, 0] = _rt(vec.float(), dt)
            return
        # family A: orthogonal queries over the step's tokens (inside the kept and inside the dropped channels for ThinK), norms
        # spread over sqrt(D) * [0.6, 1.3]; one query per head ("own" calls) or per GQA group
        shared = self.mode != "own"
        heads = hkv if shared else hq
        q = torch.zeros(b, heads, t, D, dtype=torch.float64)
        for bi in range(b):
            for h in range(heads):
                m = self.keepmask[bi, h * self.grp if shared else h]
                for part in (m, ~m):
                    dim = int(part.sum())
                    if dim == 0:
                        continue
                    x = torch.randn(dim, t, generator=g, dtype=torch.float64)
                    if dim >= t:
                        x = torch.linalg.qr(x).Q * math.sqrt(dim)
                    q[bi, h][:, part] = x.T
                q[bi, h] *= (0.6 + 0.7 * torch.rand(t, 1, generator=g, dtype=torch.float64))
        if shared:
            q = q.repeat_interleave(self.grp, 1)
        self.q = _rt(q.float(), dt)

    # -- needles --------------------------------------------------------------------------------------------------------------
    def _vec(self, b, h, i, nats, pruned=False):
        q = self.q[b, h, i].double()
        if pruned:
            q = q * self.keepmask[b, h]
        return (nats * math.sqrt(self.D) / float(q @ q)) * q

    def _write(self, b, h, r, nats, i):
        name, j = self.locate(b, h, r)
        vec = _rt(self._vec(b, h, i, nats, name == "pruned").float(), self.dtype)
        if name == "pruned":
            self.pk[b, h, j] = vec
        elif name == "prefix":
            self.ek[b, h, j] = vec
        else:
            {"qtail": self.qk, "tail": self.tk, "new": self.nk}[name][b, h // self.grp, j] = vec
        hh = h if name in ("pruned", "prefix") else h // self.grp
        if self.v_outliers and nats == NEEDLE_NATS and (name, b, hh, j) not in self._scaled:     # the needle's value row holds
            V = {"pruned": self.pv, "prefix": self.ev, "qtail": self.qv, "tail": self.tv, "new": self.nv}[name]     # outliers: |v| up to 16
            V[b, hh, j] = _rt(V[b, hh, j] * 4, self.dtype)
            self._scaled.add((name, b, hh, j))

    def _plant(self):
        b, hq, t = self.b, self.hq, self.t
        own, kv = ("pruned", "prefix"), ("qtail", "tail")
        if self.mode in ("own", "shared"):
            kinds = own if self.mode == "own" else kv
            for bi in range(b):
                for h in range(hq):
                    lane, lanes = (h, hq) if self.mode == "own" else (h // self.grp, self.hkv)
                    edges, regular = self.probe_rows(bi, h, kinds)
                    rows = edges + [r for k, r in enumerate(regular) if k % lanes == lane]
                    rows += [r for r in regular if r not in rows][:max(0, t - len(rows))]       # a row for every token where there are t
                    for i, r in enumerate(_deal(rows, self.call, t)):
                        if r is not None:
                            self.probes.append((bi, h, i, r))
        elif self.mode == "new":                                             # every new row, from its own token
            self.probes = [(bi, h, i, int(self.n[bi, h]) - t + i) for bi in range(b) for h in range(hq) for i in range(t)]
        else:                                                                # decoy in new row i + 1; the needle in a visible row
            for bi in range(b):
                for h in range(hq):
                    kinds = kv if (self.T + self.Tq) >= t else own
                    rows = [r for name, o, m in self.segments(bi, h) if name in kinds for r in range(o, o + m)]
                    for i in range(t):
                        if len(rows) >= t:
                            self.probes.append((bi, h, i, rows[-1 - i]))
                            if i + 1 < t:
                                self._write(bi, h, int(self.n[bi, h]) - t + i + 1, DECOY_NATS, i)
            if self.entry == "rows":                                         # and once behind the batch row's last prefix row
                for bi in range(b):
                    for h in range(hq):
                        p = int(self.npre[bi, h])
                        if any(pb == bi and ph == h and self.locate(pb, ph, r)[0] != "new" for pb, ph, _, r in self.probes):
                            self.ek[bi, h, p] = _rt(self._vec(bi, h, 0, DECOY_NATS).float(), self.dtype)
                            self.keep_spare[bi, h, p] = True
        for bi, h, i, r in self.probes:
            self._write(bi, h, r, NEEDLE_NATS, i)

    def n_calls(self):
        """How many "own" / "shared" calls visit every probe row of the case once."""
        kinds = ("pruned", "prefix") if self.mode == "own" else ("qtail", "tail")
        most = 0
        for bi in range(self.b):
            for h in range(self.hq):
                lanes = self.hq if self.mode == "own" else self.hkv
                edges, regular = self.probe_rows(bi, h, kinds)
                most = max(most, len(edges) + -(-len(regular) // lanes))
        return -(-most // self.t)

    # -- the entry's arguments ------------------------------------------------------------------------------------------------
    def _dense(self, k, rows, spare, poison=True):
        """[b, H, rows + spare, D] in the case dtype, the spare rows NaN."""
        out = torch.full((k.shape[0], k.shape[1], rows + spare, self.D), float("nan") if poison else 0.0)
        out[:, :, :rows] = k[:, :, :rows]
        return out.to(self.dtype)

    def _qseg(self, k, v, rows, outliers):
        """One quantized segment (and its outlier pools), written by the numpy restatement: the bytes kvc_quantize_rows[_outliers]
        writes (test_quantize_rows_bit_identical), so the same case serves the stand-ins and the device."""
        heads, G, nb = k.shape[1], self.G, self.nbits
        cap = rows + G
        kc = torch.zeros(self.b, heads, cap, self.D * nb // 8, dtype=torch.uint8)
        vc = torch.zeros_like(kc)
        km = torch.zeros(self.b, heads, -(-cap // G), 2, self.D, dtype=torch.float32)
        vm = torch.zeros(self.b, heads, cap, self.D // G, 2, dtype=torch.float32)
        ks, vs = k.to(self.dtype), v.to(self.dtype)
        if not outliers:
            if rows:
                Q.quantize_rows(ks, kc, km, 0, Q.KEYS, nb, G)
                Q.quantize_rows(vs, vc, vm, 0, Q.VALUES, nb, G)
            return (kc, vc, km, vm, rows), None
        pools = []
        thr = KQ.round_threshold(self.thr, self.dtype)
        for src, codes, meta, mode in ((ks, kc, km, Q.KEYS), (vs, vc, vm, Q.VALUES)):
            need = int(KQ.split(Q._f32(src), thr)[0].reshape(self.b, -1).sum(1).max()) if rows else 0
            pool = (torch.zeros(self.b, need + 16, dtype=torch.uint8), torch.zeros(self.b, need + 16, dtype=self.dtype),
                    torch.zeros(self.b, dtype=torch.int32), torch.zeros(self.b, heads, cap, dtype=torch.int32))
            if rows:
                KQ.quantize_rows_outliers(src, codes, meta, pool, 0, mode, nb, G, self.thr)
            pools.append(pool)
        return (kc, vc, km, vm, rows), pools

    def _finalize(self):
        e, dt, t, T, D = self.entry, self.dtype, self.t, self.T, self.D
        q, kn, vn = self.q.to(dt), self.nk.to(dt), self.nv.to(dt)
        kt, vt = self._dense(self.tk, T, t + 4), self._dense(self.tv, T, t + 4)
        kp, vp = self.ek.clone(), self.ev.clone()
        for bi in range(self.b):
            for h in range(self.hq):
                dead = torch.arange(kp.shape[2]) >= int(self.npre[bi, h])
                dead &= ~self.keep_spare[bi, h]
                kp[bi, h, dead] = float("nan")
                vp[bi, h, dead] = float("nan")
        kp, vp = kp.to(dt), vp.to(dt)
        self.kw = {}
        self.appended_into = (6, 7, T)                                        # (index of the K buffer, of the V buffer, first row)
        if e in ("step2", "scored"):
            self.args = [q, kn, vn, kp, vp, self.Pmax, kt, vt, T, self.scaling]
            if e == "scored":
                sp = torch.zeros(self.b, self.hq, self.Pmax + SPARE, dtype=torch.float32)
                st = torch.zeros(self.b, self.hq, T + t + 4, dtype=torch.float32)
                sp[:, :, self.Pmax:], st[:, :, T + t:] = 123.0, 321.0        # must stay
                if self.family == "B":
                    sp[:, :, :self.Pmax] = torch.rand(self.b, self.hq, self.Pmax, generator=self.g)
                    st[:, :, :T] = torch.rand(self.b, self.hq, T, generator=self.g)
                self.args += [sp, st, self.scaling]
                del self.args[9]
        elif e == "think":
            per = 16 // q.element_size()
            dkp = -(-self.keep // per) * per
            order = torch.sort(self.keepmask.to(torch.int8), dim=-1, descending=True, stable=True).indices[..., :self.keep]
            k_pruned = torch.gather(self.pk, 3, order[:, :, None, :].expand(-1, -1, self.P1, -1))
            k_pruned = torch.nn.functional.pad(k_pruned, (0, dkp - self.keep)).to(dt).contiguous()
            chan = torch.nn.functional.pad(order.to(torch.int16), (0, dkp - self.keep), value=-1).contiguous()
            values = torch.cat([self.pv.to(dt), vp], 2)
            self.args = [q, kn, vn, kp, values, self.Pmax, kt, vt, T, self.scaling]
            self.kw = dict(k_pruned=k_pruned, chan=chan, pruned_rows=self.P1)
        elif e == "rows":
            rows_b = torch.tensor(self.npre[:, 0], dtype=torch.int32)
            self.args = [q, kn, vn, kp, vp, rows_b, self.Pmax, kt, vt, T, self.scaling]
            self.appended_into = (7, 8, T)
        elif e in QUANTIZED:
            outl = e == "outl"
            self.pre, self.ppools = self._qseg(self.ek[:, :, :self.Pmax], self.ev[:, :, :self.Pmax], self.Pmax, outl)
            self.qt, self.tpools = self._qseg(self.qk, self.qv, self.Tq, outl)
            kr = torch.full((self.b, self.hkv, self.R + 8, D), float("nan"))
            vr = kr.clone()
            kr[:, :, :T], vr[:, :, :T] = self.tk, self.tv
            kr, vr = kr.to(dt), vr.to(dt)
            qt, tp = (self.qt, self.tpools) if self.Tq else (None, None)
            if outl:
                self.args = [q, kn, vn, self.pre, qt, self.ppools, tp, kr, vr, T, self.scaling, self.nbits, self.G, self.R]
                self.appended_into = (7, 8, T)
            else:
                self.args = [q, kn, vn, self.pre, qt, kr, vr, T, self.scaling, self.nbits, self.G, self.R]
                self.appended_into = (5, 6, T)
        else:                                                                # ragged: head h at seg_off[h], seg_len + appended rows held
            offs, row = [], 0
            for h in range(self.hq):
                offs.append(row)
                row += int(self.npre[0, h]) - self.appended + self.slack
            kf, vf = torch.full((row, D), float("nan")), torch.full((row, D), float("nan"))
            for h in range(self.hq):
                p = int(self.npre[0, h])
                kf[offs[h]:offs[h] + p], vf[offs[h]:offs[h] + p] = self.ek[0, h, :p], self.ev[0, h, :p]
            self.offs = offs
            self.args = [q, kn, vn, kf.to(dt), vf.to(dt), torch.tensor(offs, dtype=torch.int64),
                         torch.tensor(self.npre[0] - self.appended, dtype=torch.int32), self.appended, self.scaling]
            self.kw = dict(slack=self.slack)
            self.appended_into = None

    def expected_buffers(self):
        """The arguments as they must be after the call: the step's rows appended, nothing else changed (scores aside)."""
        exp = _clone(self.args)
        kn, vn = self.args[1], self.args[2]
        if self.entry == "ragged":
            for h in range(self.hq):
                o = self.offs[h] + int(self.npre[0, h])
                exp[3][o:o + self.t], exp[4][o:o + self.t] = kn[0, h // self.grp], vn[0, h // self.grp]
        else:
            ki, vi, r0 = self.appended_into
            exp[ki][:, :, r0:r0 + self.t], exp[vi][:, :, r0:r0 + self.t] = kn, vn
        return exp

    # -- the virtual cache ----------------------------------------------------------------------------------------------------
    def _assemble(self, kv_map="div", patch_k=True, npre=None):
        """K, V [b, hq, nmax, D] fp64 as the kernel is to see them (restated de-quantization for the quantized segments).
        kv_map / patch_k / npre exist for the mutants: KV head h % H_kv instead of h / group, key outliers left unpatched, other
        prefix lengths."""
        b, hq, D = self.b, self.hq, self.D
        npre = self.npre if npre is None else npre
        n = self.P1 + npre + self.Tq + self.T + self.t
        nmax = int(n.max())
        K, V = np.zeros((b, hq, nmax, D)), np.zeros((b, hq, nmax, D))
        quantized = np.zeros((b, hq, nmax), dtype=bool)
        pre_k, pre_v, qt_k, qt_v = self.ek, self.ev, self.qk, self.qv
        if self.entry in QUANTIZED:
            def restated(seg, pools):
                if self.entry == "quant":
                    return Q.segment_values(seg, self.nbits, self.G)
                k, v = KQ.segment_values(seg, pools, self.nbits, self.G)
                if not patch_k:
                    k = Q.segment_values(seg, self.nbits, self.G)[0]
                return k, v
            pre_k, pre_v = restated(self.pre, self.ppools)
            if self.Tq:
                qt_k, qt_v = restated(self.qt, self.tpools)
        kvh = (lambda h: h // self.grp) if kv_map == "div" else (lambda h: h % self.hkv)
        pkz = self.pk * self.keepmask[:, :, None, :]
        for bi in range(b):
            for h in range(hq):
                g, p = kvh(h), int(npre[bi, h])
                ks = [pkz[bi, h], pre_k[bi, h, :p], qt_k[bi, g], self.tk[bi, g], self.nk[bi, g]]
                vs = [self.pv[bi, h], pre_v[bi, h, :p], qt_v[bi, g], self.tv[bi, g], self.nv[bi, g]]
                m = int(n[bi, h])
                K[bi, h, :m], V[bi, h, :m] = _np64(torch.cat(ks, 0)), _np64(torch.cat(vs, 0))
                if self.entry in QUANTIZED:
                    quantized[bi, h, self.P1:self.P1 + p + self.Tq] = True
        if kv_map == "div" and patch_k and npre is self.npre:
            self.K, self.V, self.quantized = K, V, quantized
        return K, V, n

    def ref64(self):
        return attention64(_np64(self.q), self.K, self.V, self.n, self.scaling)

    def ref32(self):
        """The plain fp32 torch restatement over the same virtual cache.  [b, hq, t, D] fp64 holding fp32 values."""
        q, K, V = (torch.from_numpy(np.asarray(x)).float() for x in (_np64(self.q), self.K, self.V))
        out = torch.zeros(self.b, self.hq, self.t, self.D)
        for bi in range(self.b):
            for h in range(self.hq):
                for i in range(self.t):
                    vis = int(self.n[bi, h]) - self.t + i + 1
                    w = torch.softmax((K[bi, h, :vis] @ q[bi, h, i]) * self.scaling, -1)
                    out[bi, h, i] = w @ V[bi, h, :vis]
        return out.double().numpy()

    # -- running --------------------------------------------------------------------------------------------------------------
    def run(self, fn, device=None):
        """fn(*args, **kw) on copies of the arguments (moved to `device`).  -> (out [b, hq, t, D] fp64 numpy, arguments after)."""
        args, kw = _clone(self.args, device), _clone(self.kw, device)
        if self.q_view:                                                      # the transposed view the model hands over
            args[0] = args[0].transpose(1, 2).contiguous().transpose(1, 2)
        out = fn(*args, **kw)
        if device is not None:
            torch.cuda.synchronize()
        assert out.shape == (self.b, self.t, self.hq, self.D) and out.dtype == self.dtype
        return _np64(out.transpose(1, 2)), _clone(args, "cpu")

    # -- checks ---------------------------------------------------------------------------------------------------------------
    def check_condition(self):
        """Family A: every probe's off-needle weight in fp64 on the restated cache is <= 2^-40."""
        _, p = self.ref64()
        worst, self.off = 0.0, {}
        for bi, h, i, r in self.probes:
            row = p[bi, h, i].copy()
            row[r] = 0.0
            off = float(row.sum())
            worst = max(worst, off)
            self.off[(bi, h, i, r)] = off
            if not off <= OFF_WEIGHT or not p[bi, h, i, r] > 0.5:
                raise ProbeInputError(f"probe {self.describe(bi, h, i, r)}: off-needle weight {off:.3e} > 2^-40")
        return worst

    def describe(self, bi, h, i, r):
        name, j = self.locate(bi, h, r)
        return f"(b={bi}, h={h}, token={i}, virtual row {r} = {name} row {j} of {int(self.n[bi, h])} rows)"

    def check_needles(self, out):
        """out[b, h, i] == V[r*] bit for bit (unquantized entries) or within 1 ulp of the dtype (quantized entries).
        A de-quantized value row, unlike the drawn ones, can hold an element that is 0 or tiny against the rest (a 2-bit code in the
        middle of a group that straddles 0), where the other rows' weight shows below 1 ulp: there the quantized entries are also
        allowed what those rows can add, 4 x the probe's own off-needle weight in fp64 (<= 2^-40, about 1e-32 in practice; the 4
        covers fp32 logits) x the head's largest |v|."""
        assert self.probes, "a needle call without probes"
        if not hasattr(self, "off"):
            self.check_condition()
        bad = []
        for bi, h, i, r in self.probes:
            want = _np64(torch.from_numpy(self.V[bi, h, r]).to(self.dtype))
            got = out[bi, h, i]
            if self.entry in QUANTIZED:
                leak = 4.0 * self.off[(bi, h, i, r)] * float(np.abs(self.V[bi, h, :int(self.n[bi, h])]).max())
                ok = bool((np.abs(got - want) <= ulp(want, self.dtype) + leak).all())
            else:
                ok = np.array_equal(got, want)
            if not ok:
                bad.append(self.describe(bi, h, i, r))
        assert not bad, f"{len(bad)} of {len(self.probes)} needles missed, first: {bad[:3]}"
        return len(self.probes)

    def check_scores(self, after):
        """Scored step, family A: the score of r* grows by 1 per token probing it (within 2^-23), all other rows of the head
        together by <= 2^-30; nothing at or past the visible rows changes."""
        sp, st = after[9].double().numpy(), after[10].double().numpy()
        P, T, t = self.Pmax, self.T, self.t
        assert (sp[:, :, P:] == 123.0).all() and (st[:, :, T + t:] == 321.0).all(), "score rows past the visible ones changed"
        got = np.concatenate([sp[:, :, :P], st[:, :, :T + t]], 2)
        want = np.zeros_like(got)
        for bi, h, i, r in self.probes:
            want[bi, h, r] += 1.0
        for bi in range(self.b):                                             # heads whose every token has a needle
            for h in range(self.hq):
                if len([1 for pb, ph, _, _ in self.probes if (pb, ph) == (bi, h)]) == t:
                    hit = want[bi, h] > 0
                    assert (np.abs(got[bi, h] - want[bi, h])[hit] <= 2.0 ** -23 * want[bi, h][hit]).all(), \
                        f"b={bi} h={h}: a needle's score did not grow by 1 per probing token"
                    assert float(np.abs(got[bi, h][~hit]).sum()) <= 2.0 ** -30, f"b={bi} h={h}: the other rows' scores grew"

    def check_buffers(self, after):
        """Appended rows byte-identical, nothing else in any buffer changed (score buffers are check_scores')."""
        exp = self.expected_buffers()
        skip = (9, 10) if self.entry == "scored" else ()
        for k, (a, e) in enumerate(zip(after, exp)):
            if k not in skip:
                _same_bytes(a, e, f"argument {k}")
        if self.entry == "scored":
            sp, st = after[9], after[10]
            assert (sp[:, :, self.Pmax:] == 123.0).all() and (st[:, :, self.T + self.t:] == 321.0).all()

    def bound(self):
        """Family B: (ref64, e_ref, sum_j p_j |v_j|)."""
        ref, p = self.ref64()
        pv = np.einsum("bhtr,bhrd->bhtd", p, np.abs(self.V))
        e_ref = float((np.abs(self.ref32() - ref) / pv).max())
        if self.entry in QUANTIZED:                                          # the de-quantization may be 1 fp32 ulp off
            q = _np64(self.q)
            dK = np.where(self.quantized[..., None], ulp(self.K, torch.float32), 0.0)
            dV = np.where(self.quantized[..., None], ulp(self.V, torch.float32), 0.0)
            for sgn in (1.0, -1.0):
                for i in range(self.t):                                      # worst signs for token i's logits
                    Ks = self.K + sgn * dK * np.sign(q[:, :, i])[:, :, None, :]
                    shifted, _ = attention64(q, Ks, self.V + sgn * dV, self.n, self.scaling)
                    e_ref = max(e_ref, float((np.abs(shifted - ref) / pv)[:, :, i].max()))
        return ref, e_ref, pv

    def check_bound(self, out):
        """-> (e_kernel, e_ref); asserts the per-element bound at factor 4."""
        ref, e_ref, pv = self.bound()
        err = np.abs(out - ref)
        half = 0.5 * ulp(np.maximum(np.abs(ref), np.abs(out)), self.dtype)
        e_kernel = float((np.maximum(0.0, err - half) / pv).max())
        over = err > half + FACTOR * e_ref * pv
        assert not over.any() and np.isfinite(out).all(), \
            f"{int(over.sum())} elements outside the bound: e_kernel / e_ref = {e_kernel / e_ref:.2f} (e_ref {e_ref:.3e})"
        return e_kernel, e_ref


def _deal(rows, call, t):
    """The rows the t tokens of call number `call` probe: token i takes list entry call + i * ceil(len / t), so the tokens of a head
    sit far apart; a token whose entry is past the end takes a row no other token of the call has (None if there is none)."""
    nc = max(1, -(-len(rows) // t))
    pick = [rows[call % nc + i * nc] if call % nc + i * nc < len(rows) else None for i in range(t)]
    spare = [r for r in rows if r not in pick]
    return [r if r is not None else (spare.pop() if spare else None) for r in pick]


def _clone(x, device=None):
    if torch.is_tensor(x):
        return x.clone() if device is None else x.to(device).clone()
    if isinstance(x, (list, tuple)):
        return type(x)(_clone(y, device) for y in x)
    if isinstance(x, dict):
        return {k: _clone(v, device) for k, v in x.items()}
    return x


def _same_bytes(a, e, what):
    if torch.is_tensor(e):
        assert a.shape == e.shape and a.dtype == e.dtype, what
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[e.element_size()]
        assert torch.equal(a.contiguous().view(it), e.contiguous().view(it)), f"{what} changed where it must not (or misses the appended rows)"
    elif isinstance(e, (list, tuple)):
        for k, (x, y) in enumerate(zip(a, e)):
            _same_bytes(x, y, f"{what}[{k}]")
    else:
        assert a == e, what


# ---- needle calls of a case ------------------------------------------------------------------------------------------------
def needle_calls(spec, seed=0):
    """Every family-A case of a spec: own calls, shared calls, the new rows, the decoys (t > 1)."""
    out = []
    for mode in ("own", "shared"):
        first = Case(spec, "A", seed, mode, 0)
        if not first.probes:
            continue
        out.append(first)
        out += [Case(spec, "A", seed + 1000 * c, mode, c) for c in range(1, first.n_calls())]
    out.append(Case(spec, "A", seed + 7, "new"))
    if spec["t"] > 1:
        out.append(Case(spec, "A", seed + 8, "decoy"))
    return out


# ---- the ragged stand-in -----------------------------------------------------------------------------------------------------
def standin_ragged_decode_step(q, k_new, v_new, k_flat, v_flat, seg_off, seg_len, appended, scaling, slack=0):
    """What kvc_ragged_decode_step computes, in fp32 torch: the step's rows behind every head's segment, per-head attention."""
    b, hq, t, D = q.shape
    grp = hq // k_new.shape[1]
    out = torch.empty(b, t, hq, D, dtype=q.dtype)
    for hb in range(b * hq):
        bi, h = divmod(hb, hq)
        o, n = int(seg_off[hb]), int(seg_len[hb]) + appended
        k_flat[o + n:o + n + t], v_flat[o + n:o + n + t] = k_new[bi, h // grp], v_new[bi, h // grp]
        for i in range(t):
            K, V = k_flat[o:o + n + i + 1].float(), v_flat[o:o + n + i + 1].float()
            out[bi, i, h] = (torch.softmax((K @ q[bi, h, i].float()) * scaling, -1) @ V).to(q.dtype)
    return out


# ---- deliberately wrong restatements (CPU only): the checker must reject them ---------------------------------------------
MUTANTS = ("drop_segment_last", "drop_split_first", "double_count", "see_extra_new_row", "tail_wrong_kv_head", "v_shift_in_block",
           "combine_forgets_rescale", "rows_b_off_by_one", "skip_outlier_patch_k")


def mutant_applies(case, name):
    splits = split_plan(case.b, case.hq, case.t, int(case.n.max()))[0]
    return {"drop_split_first": splits > 1, "combine_forgets_rescale": splits > 1 and case.entry != "ragged",
            "see_extra_new_row": case.t > 1, "tail_wrong_kv_head": case.grp > 1 and case.hkv > 1 and case.entry != "ragged",
            "rows_b_off_by_one": case.entry == "rows", "skip_outlier_patch_k": case.entry == "outl"}.get(name, True)


def mutant_out(case, name):
    """The output [b, hq, t, D] (fp64 holding dtype values) of a decode step that is wrong in the way `name` says, in fp64."""
    assert name in MUTANTS and mutant_applies(case, name)
    K, V, n = case.K, case.V, case.n
    if name == "tail_wrong_kv_head":
        K, V, n = case._assemble(kv_map="mod")
    elif name == "skip_outlier_patch_k":
        K, V, n = case._assemble(patch_k=False)
    elif name == "rows_b_off_by_one":
        K, V, n = case._assemble(npre=np.maximum(case.npre - 1, 0))
    q = _np64(case.q)
    t = case.t
    out = np.zeros((case.b, case.hq, t, case.D))
    _, rps = split_plan(case.b, case.hq, t, int(case.n.max()))
    for bi in range(case.b):
        for h in range(case.hq):
            Vh = V[bi, h]
            if name == "v_shift_in_block":
                Vh = Vh.copy()
                lo = 64 if n[bi, h] >= 128 else 0
                hi = min(lo + 64, int(n[bi, h]) - t)
                Vh[lo:hi] = np.roll(V[bi, h, lo:hi], -1, axis=0)
            for i in range(t):
                vis = int(n[bi, h]) - t + i + 1
                if name == "see_extra_new_row" and i + 1 < t:
                    vis += 1
                s = (K[bi, h, :vis] @ q[bi, h, i]) * case.scaling
                if name == "drop_segment_last":
                    for seg, o, rows in case.segments(bi, h):
                        if seg != "new":
                            s[o + rows - 1] = -np.inf
                elif name == "drop_split_first":
                    s[rps:vis:rps] = -np.inf
                elif name == "double_count":
                    s[0:vis:64] += math.log(2.0)
                if name == "combine_forgets_rescale":
                    acc, l = np.zeros(case.D), 0.0
                    M = s.max()
                    for k, r0 in enumerate(range(0, vis, rps)):
                        sl = s[r0:r0 + rps]
                        ref = sl.max() if k == 1 else M                      # split 1 is merged as if its maximum were the global one
                        w = np.exp(sl - ref)
                        acc, l = acc + w @ Vh[r0:r0 + len(sl)], l + w.sum()
                    out[bi, h, i] = acc / l
                else:
                    w = np.exp(s - s.max())
                    out[bi, h, i] = (w / w.sum()) @ Vh[:vis]
    return _np64(torch.from_numpy(out).to(case.dtype))


def mutant_scores_double_count(case):
    """The arguments after a scored step that counts every row at a multiple of 64 twice: each copy of such a row holds half of
    the row's probability and the score receives one copy's (a needle's score grows by 1/2, not 1)."""
    assert case.entry == "scored"
    q = _np64(case.q)
    after = _clone(case.expected_buffers())
    sp, st = after[9], after[10]
    for bi in range(case.b):
        for h in range(case.hq):
            for i in range(case.t):
                vis = int(case.n[bi, h]) - case.t + i + 1
                s = (case.K[bi, h, :vis] @ q[bi, h, i]) * case.scaling
                s[0:vis:64] += math.log(2.0)
                w = np.exp(s - s.max())
                w /= w.sum()
                w[0:vis:64] /= 2
                w = torch.from_numpy(w).float()
                sp[bi, h, :case.Pmax] += w[:case.Pmax]
                st[bi, h, :vis - case.Pmax] += w[case.Pmax:]
    return after


# ---- the grid both conformance files run ------------------------------------------------------------------------------------
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
COMBOS = [(BF16, 128), (BF16, 64), (FP16, 128), (FP16, 64), (FP32, 128), (FP32, 64)]
HEADS = [(8, 2), (4, 4), (8, 2), (4, 1), (8, 8), (8, 2)]
RAGGED_LENS = [8, 9, 40, 133, 64, 17, 2100, 777]


def _grid():
    """Every template instantiation of the six kernels (3 dtypes x 2 head dims, x 3 code widths for the quantized ones), each dtype
    and head dim without splits (<= 64 rows) and with them; total rows about 40, 130, 2 357 and 4 105, t in {1, 3, 5}."""
    out = []
    for k, (dt, D) in enumerate(COMBOS):
        hq, hkv = HEADS[k]
        t_s, t_l = (1, 3, 5)[k % 3], (1, 5, 3)[k % 3]                   # one token at 130 rows, five at 2 357, three at 4 105
        rows_l = (130, 2357, 4105)[k % 3]
        T_l = (27, 300, 37)[k % 3]
        b2 = 1 + k % 2
        base = dict(dtype=dt, D=D, hq=hq, hkv=hkv)
        for e in ("step2", "scored"):
            out.append(dict(base, entry=e, b=b2 if e == "step2" else 1, t=t_s, P=40 - 9 - t_s, T=9))
            out.append(dict(base, entry=e, b=3 - b2 if e == "step2" else 1, t=t_l, P=rows_l - T_l - t_l, T=T_l, q_view=k == 1))
        keep = 45 if D == 64 else (77, 90, 128)[k // 2]
        out.append(dict(base, entry="think", t=t_s, P1=20, keep=keep, P=8, T=12 - t_s))
        out.append(dict(base, entry="think", t=t_l, P1=rows_l - 32 - T_l - t_l, keep=keep, P=32, T=T_l, q_view=k == 1))
        out.append(dict(base, entry="rows", b=4, t=t_s, P=[0, 1, 30, 40], T=9))
        out.append(dict(base, entry="rows", b=6, t=t_l, P=[0, 1, 63, 64, 65, rows_l - T_l - t_l], T=T_l, q_view=k == 1))
        for step in (0, 1):
            out.append(dict(base, entry="ragged", hq=8, hkv=HEADS[k][1] if HEADS[k][0] == 8 else 2, t=t_l, appended=step * t_l,
                            P=[x + step * t_l for x in RAGGED_LENS], slack=2 * t_l + 1, q_view=k == 1 and step == 1))
        for j, nbits in enumerate((2, 4, 8)):
            G = [g for g in (32, 64, 128) if g <= D][(k + j) % (2 if D == 64 else 3)]
            R = max(G, 64)
            short = j == 0 or (j == 2 and k % 2 == 0)                       # 2 bits without splits, 4 bits with, 8 bits alternating
            res = (0, R - 1, 5)[(k + 2 * j) % 3]                             # residual empty, one row short of residual_length, a few
            t = t_s if short else t_l
            if short:
                Tq = G if G == 32 and (k + j) % 2 == 0 else 0
                res = min(res, 7)
                P = max(12, 40 - Tq - res - t)                               # a partial (only) key group
            else:
                Tq = (0, G, 3 * G)[(k + j) % 3]
                if rows_l - Tq - res - t < G:
                    Tq = 0
                P = rows_l - Tq - res - t
                P -= 3 if P % G == 0 else 0                                  # a partial last key group
            for e in QUANTIZED:
                out.append(dict(base, entry=e, b=b2 if j == 0 else 1, t=t, P=P, Tq=Tq, T=res, nbits=nbits, G=G, R=R,
                                q_view=k == 1 and j == 1, v_outliers=e == "outl" and j == 1 and k == 0))
    # few heads: 64 workgroups per head launched (4 093 rows), and decode_splits' cap of 64 biting (4 163 rows: 65 blocks of 64)
    out.append(dict(entry="step2", dtype=BF16, D=128, hq=4, hkv=1, b=1, t=3, P=4030, T=60))
    out.append(dict(entry="step2", dtype=BF16, D=128, hq=4, hkv=1, b=1, t=3, P=4100, T=60))
    return out


def spec_id(s):
    p = s["P"] if isinstance(s["P"], int) else "x".join(str(x) for x in s["P"][-3:])
    q = f"-{s['nbits']}b-G{s['G']}-Tq{s['Tq']}" if s["entry"] in QUANTIZED else ""
    return f"{s['entry']}-{str(s['dtype'])[6:]}-D{s['D']}-h{s['hq']}x{s['hkv']}-b{s.get('b', 1)}-t{s['t']}-P{p}-T{s.get('T', 0)}{q}" + \
        (f"-P1_{s['P1']}" if s.get("P1") else "") + (f"-app{s['appended']}" if s.get("appended") else "") + ("-qview" if s.get("q_view") else "")


GRID = _grid()


def splits_of(spec):
    """The split count the kernels plan for a spec (1 for the ragged kernel, which has no split path)."""
    if spec["entry"] == "ragged":
        return 1
    rows = spec.get("P1", 0) + int(np.max(spec["P"])) + spec.get("Tq", 0) + spec.get("T", 0) + spec["t"]
    return split_plan(spec.get("b", 1), spec["hq"], spec["t"], rows)[0]
