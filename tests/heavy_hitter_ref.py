"""TEST-ONLY restatements of the heavy-hitter rules (include/kvc.h: kvc_decode_step_scored, kvc_decode_evict) in torch, on whatever
device the tensors live on, and CPU stand-ins for the two `_kvc` helpers so the layer's bookkeeping runs without a GPU.  Never shipped.

Rule 2 (a decode step): for each new token i in ascending order and each row r visible to it (its own row included)
score[h][r] += softmax_r(q_i[h] . K[h][r] * scaling); a row appended by the step starts from 0.
Rule 3 (an eviction): the k rows topk(score[h][0 : S - W], k) picks, in top-k order, then the last W rows; K, V and scores."""
import torch


def virtual_rows(pre, tail, P, T, G):
    """[b, H_q, P + T, ...]: prefix row r of query head h for r < P, else tail row r - P of KV head h / G."""
    return torch.cat([pre[:, :, :P], tail[:, :, :T].repeat_interleave(G, 1)], 2)


def step_probs(q, k_prefix, k_tail, P, T, scaling, dtype=torch.float64):
    """Per new token i the softmax [b, H_q, P + T + i + 1] of rule 2, computed in `dtype`.  k_tail already holds the step's rows at
    [T, T + t)."""
    b, hq, t, D = q.shape
    G = hq // k_tail.shape[1]
    K = virtual_rows(k_prefix, k_tail, P, T + t, G).to(dtype)
    out = []
    for i in range(t):
        logits = torch.einsum("bhd,bhrd->bhr", q[:, :, i].to(dtype), K[:, :, :P + T + i + 1]) * scaling
        out.append(torch.softmax(logits, -1))
    return out


def step_increment(probs, rows):
    """sum_i p_i, zero-padded to `rows` columns, in the dtype of the probabilities."""
    inc = torch.zeros(*probs[0].shape[:2], rows, dtype=probs[0].dtype, device=probs[0].device)
    for p in probs:
        inc[:, :, :p.shape[2]] += p
    return inc


def max_rel_err(x, ref64):
    return float(((x.to(torch.float64) - ref64).abs() / ref64).max())


def one_step_bound(q, k_prefix, k_tail, P, T, scaling):
    """(probs64, e_ref): the fp64 restatement and the maximum relative error against it of the plain fp32 torch restatement on
    the same tensors, both taken on the step's increment sum_i p_i over every visible row.  The kernel differs from the fp32
    restatement only by the order of the dot product's sum and by the hardware exp2, so its own maximum relative error must stay
    within 4 x e_ref.  Every fp64 probability must exceed 1e-12 so that a
    relative error means something on every row (asserted here)."""
    p64 = step_probs(q, k_prefix, k_tail, P, T, scaling, torch.float64)
    p32 = step_probs(q, k_prefix, k_tail, P, T, scaling, torch.float32)
    assert all(float(p.min()) > 1e-12 for p in p64), min(float(p.min()) for p in p64)
    rows = p64[-1].shape[2]
    return p64, max_rel_err(step_increment(p32, rows), step_increment(p64, rows))


def check_step(before, after, p64, e_ref, t_new_from):
    """The scores `after` a step against rule 2 in fp64 from the scores `before` ([b, H_q, rows] fp32 each; columns at or past
    t_new_from are the step's own rows and start from 0).  Bound per element, with inc = sum_i p_i in fp64:
        |after - (before + inc)| <= 4 * e_ref * inc  +  t * 2^-24 * (before + inc)
    — the first term is the one-step bound on the probabilities, the second the t fp32 additions onto the running sum (each
    rounds to within half an ulp of a value that never exceeds the final sum).  Returns the kernel's maximum relative error of
    the increment where before == 0 (there the second term is part of the increment itself)."""
    rows = after.shape[2]
    b0 = before.to(torch.float64).clone()
    b0[:, :, t_new_from:] = 0
    inc = step_increment(p64, rows)
    want = b0 + inc
    err = (after.to(torch.float64) - want).abs()
    bound = 4 * e_ref * inc + len(p64) * 2.0 ** -24 * want
    assert bool((err <= bound).all()), (float((err / bound.clamp_min(1e-300)).max()), e_ref)
    zero = b0 == 0
    return float((err[zero] / inc[zero]).max()) if bool(zero.any()) else 0.0


def evict_reference(K, V, score, W, k, tie_mode):
    """Rule 3 on the CPU: K, V [b, H_q, S, D], score [b, H_q, S] fp32 -> (K', V', score', idx).  torch_cpu: torch.topk's own order
    and membership of equal scores; canonical: value descending, index ascending."""
    K, V, score = K.cpu(), V.cpu(), score.cpu()
    S = score.shape[2]
    cand = score[:, :, :S - W]
    if tie_mode in ("torch_cpu", 0):
        idx = torch.topk(cand, k, dim=-1).indices
    else:
        idx = torch.sort(cand, dim=-1, descending=True, stable=True).indices[:, :, :k]
    rows = torch.cat([idx, torch.arange(S - W, S).expand(*idx.shape[:2], W)], 2)
    g = rows[..., None].expand(-1, -1, -1, K.shape[3])
    return K.gather(2, g), V.gather(2, g), score.gather(2, rows), idx


# ---- CPU stand-ins for the layer's two kernels ---------------------------------------------------------------------------------
def standin_decode_step_scored(q, k_new, v_new, k_prefix, v_prefix, prefix_rows, k_tail, v_tail, tail_rows, score_prefix, score_tail,
                               scaling, ws=None):
    b, hq, t, D = q.shape
    P, T, G = prefix_rows, tail_rows, hq // k_new.shape[1]
    k_tail[:, :, T:T + t] = k_new
    v_tail[:, :, T:T + t] = v_new
    score_tail[:, :, T:T + t] = 0
    probs = step_probs(q, k_prefix, k_tail, P, T, scaling, torch.float32)
    V = virtual_rows(v_prefix, v_tail, P, T + t, G).float()
    outs = []
    for i, p in enumerate(probs):
        score_prefix[:, :, :P] += p[:, :, :P]
        score_tail[:, :, :T + i + 1] += p[:, :, P:]
        outs.append(torch.einsum("bhr,bhrd->bhd", p, V[:, :, :P + T + i + 1])[:, :, None])
    return torch.cat(outs, 2).transpose(1, 2).to(q.dtype)


EVICTIONS = []


def standin_decode_evict(k_prefix, v_prefix, prefix_rows, k_tail, v_tail, tail_rows, score_prefix, score_tail, out, score_out, window,
                         n_keep, tie_mode="torch_cpu", return_indices=False):
    kb, vb = out
    P, T, G = prefix_rows, tail_rows, kb.shape[1] // k_tail.shape[1]
    for o in (kb, vb, score_out):                                      # the output never aliases the input
        assert all(o.data_ptr() != x.data_ptr() for x in (k_prefix, v_prefix, k_tail, v_tail, score_prefix, score_tail))
    K, V = virtual_rows(k_prefix, k_tail, P, T, G), virtual_rows(v_prefix, v_tail, P, T, G)
    score = torch.cat([score_prefix[:, :, :P], score_tail[:, :, :T]], 2)
    ko, vo, so, idx = evict_reference(K, V, score, window, n_keep, tie_mode)
    rows = n_keep + window
    kb[:, :, :rows].copy_(ko)
    vb[:, :, :rows].copy_(vo)
    score_out[:, :, :rows].copy_(so)
    EVICTIONS.append(dict(P=P, T=T, K=K, V=V, score=score, idx=idx))
    res = (kb[:, :, :rows], vb[:, :, :rows], score_out[:, :, :rows])
    return res + (idx,) if return_indices else res


def standin_compress(method, q, k, v, window, n_keep, kernel_size=5, pooling="avgpool", tie_mode="torch_cpu", n_q_heads=None,
                     return_indices=False, return_scores=False, dot_mode=None, out=None):
    """_kvc.compress through the CPU oracle, with the caller's output buffers."""
    from cpu_compress import oracle_compress
    r = list(oracle_compress(method, q, k, v, window, n_keep, kernel_size, pooling, tie_mode, n_q_heads, return_indices, return_scores))
    if out is not None:
        rows = r[0].shape[2]
        out[0][:, :, :rows].copy_(r[0])
        out[1][:, :, :rows].copy_(r[1])
        r[0], r[1] = out[0][:, :, :rows], out[1][:, :, :rows]
    return tuple(r)
