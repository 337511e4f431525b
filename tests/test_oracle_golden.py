"""The CPU oracle against the golden vectors generated from the imported reference
(oracle/gen_golden.py -> tests/golden).  This is what pins the oracle: SURVEY.md §8c.

  * A7 (top-k incl. tie order, both libstdc++ regimes) and A8 (gather + window tail) are checked
    BIT-EXACT on the reference's own intermediate scores / indices;
  * A1-A5 are checked end to end: bit-exact score count within a stated flip budget for bf16/fp16,
    a few ulp for fp32 (torch's GEMM order and its softmax exp are opaque third-party arithmetic);
  * the full pipeline's indices and K'/V' hashes are compared with the reference's.
"""
import functools

import pytest
import torch

import golden_util as G

SCORED = lambda m: m["method"] in ("snapkv", "pyramidkv", "h2o") and not m["passthrough"]          # noqa: E731
RAGGED = lambda m: m["method"] in ("adakv", "headkv")                               # noqa: E731
SMALL = lambda m: SCORED(m) and m["L"] <= 1100                                      # noqa: E731
CPU_BIG = ["C2_snapkv_8k_bf16", "C4_pyramidkv_8k_layer0", "C4_pyramidkv_8k_layer16"]   # (C3 H2O 8k: GPU suite)


@functools.lru_cache(maxsize=2)
def _cached_inputs(key):
    return G.inputs(dict(key))


def _inputs(meta):
    key = tuple(sorted((k, meta.get(k)) for k in ("Hq", "Hkv", "L", "D", "dtype", "seed", "peaky", "zero_q", "scale_q")))
    return _cached_inputs(key)


@pytest.mark.parametrize("name", G.names(SMALL))
def test_topk_on_reference_scores_is_bit_exact(oracle, name):
    """A7: libstdc++ partial_sort / nth_element+sort restatement == torch-CPU topk, ties included."""
    m, arr = G.MANIFEST[name], G.arrays(name)
    sc = G.from_bits(arr["scores"], G.DT[m["dtype"]]).contiguous()
    idx, val = oracle.topk(sc, m["n_keep"], oracle.TIES_TORCH)
    assert torch.equal(idx, torch.from_numpy(arr["indices"]))
    assert torch.equal(G.bits(val), torch.from_numpy(arr["values"]))


@pytest.mark.parametrize("name", G.names(SMALL) + CPU_BIG)
def test_gather_on_reference_indices_is_bit_exact(oracle, name):
    """A8: gather + window tail reproduces the reference's K', V' byte for byte (SHA-256)."""
    m, arr = G.MANIFEST[name], G.arrays(name)
    q, k, v = _inputs(m)
    idx = torch.from_numpy(arr["indices"])
    assert G.sha(oracle.gather(k, idx, m["W"], m["Hq"])) == m["k_out_sha256"]
    assert G.sha(oracle.gather(v, idx, m["W"], m["Hq"])) == m["v_out_sha256"]
    # GQA-native input (one copy per KV head) must give the same bytes
    g = m["Hq"] // m["Hkv"]
    assert G.sha(oracle.gather(k[:, ::g].contiguous(), idx, m["W"], m["Hq"])) == m["k_out_sha256"]


# ref_like restates the dot product with an fp64 accumulator.  torch's fp32 GEMM is the fmaf chain (0 mismatches), and
# at |logit| ~ 500 one fp32 unit of a logit (6e-5 nats) moves a probability by ~ 500 of its own units: on the fp32 fixture with
# logits that wide only the product mode (the chain) can hold the 32-unit bar, and does.
REF_LIKE_NA = ("edge_fp32_deep_underflow",)


@pytest.mark.parametrize("name,mode", [(n, md) for n in G.names(SMALL) for md in ("product", "ref_like")
                                       if not (md == "ref_like" and n in REF_LIKE_NA)])
def test_scores_against_reference(oracle, name, mode):
    """A1-A5 (A10 for H2O).  Tolerance: bf16/fp16 — at most max(2, 0.5%) of the pooled scores may differ, each by
    exactly 1 unit in the last place (a 1-ulp flip of a rounded logit/probability); fp32 — every score within
    32 fp32 ulps (torch's softmax exp differs from exp_u20 in the last bits and nothing rounds it away)."""
    m, arr = G.MANIFEST[name], G.arrays(name)
    q, k, v = _inputs(m)
    modes = G.product_modes(oracle, m) if mode == "product" else dict(dot_mode=oracle.DOT_F64, sum_mode=oracle.SUM_TORCH16)
    sc = oracle.scores(q, k, m["W"], m["kernel"], G.pool_name(m) or "avgpool", full_rows=m["method"] == "h2o", **modes)
    ref = G.from_bits(arr["scores"], G.DT[m["dtype"]])
    d = G.ulp_diff(sc, ref)
    if m["dtype"] == "fp32":
        assert int(d.max()) <= 32
    else:
        assert int(d.max()) <= 1
        assert int((d > 0).sum()) <= max(2, d.numel() // 200)


@pytest.mark.parametrize("name", G.names(SMALL) + CPU_BIG)
def test_end_to_end_indices_and_kv(oracle, name):
    """Whole update_kv in the product's arithmetic (fmaf-chain dot, kvc sum order, torch-CPU ties).
    bf16/fp16: indices and K'/V' identical to the reference on every fixture.  fp32: a head may differ only
    where two fp32 scores are within a few ulp of each other (documented: 'parity within tolerance')."""
    m, arr = G.MANIFEST[name], G.arrays(name)
    q, k, v = _inputs(m)
    ko, vo, idx, sc = oracle.compress(q, k, v, m["W"], m["n_keep"], m["kernel"], G.pool_name(m) or "avgpool",
                                      full_rows=m["method"] == "h2o", tie_mode=oracle.TIES_TORCH,
                                      **G.product_modes(oracle, m))
    ref_idx = torch.from_numpy(arr["indices"])
    heads_equal = int((idx == ref_idx).all(-1).sum())
    # every fixture, fp32 included (round 2 allowed one fp32 head to differ: with torch's 16-lane row-sum order none does)
    assert heads_equal == m["Hq"]
    assert G.sha(ko) == m["k_out_sha256"] and G.sha(vo) == m["v_out_sha256"]


@pytest.mark.parametrize("name", G.names(lambda m: m["method"] == "pyramidkv_all_layers"))
def test_every_layer_budget_vs_reference(oracle, name):
    """A9 at the config sizes, ALL 32 layers (C4: 8k, budgets 234 .. 17; C5: Mistral 32k, budgets 3978 .. 103): the schedule, and
    the oracle's top-k on its own product-mode scores against the reference's indices of every layer — each budget cuts the
    tie groups somewhere else and half of them run the other libstdc++ regime."""
    m, arr = G.MANIFEST[name], G.arrays(name)
    q, k, v = _inputs(m)
    sc = oracle.scores(q, k, m["W"], m["kernel"], m["pooling"], **G.product_modes(oracle, m))
    for layer in range(m["n_layers"]):
        lm = m["layers"][str(layer)]
        assert oracle.pyramid_k(m["cap"], m["W"], m["L"], layer, m["n_layers"]) == lm["n_keep"]
        idx, _ = oracle.topk(sc, lm["n_keep"], oracle.TIES_TORCH)
        assert torch.equal(idx, torch.from_numpy(arr[f"indices_L{layer}"].astype("int64"))), layer
        if layer in (0, 13, 31):
            assert G.sha(oracle.gather(k, idx, m["W"], m["Hq"])) == lm["k_out_sha256"]
            assert G.sha(oracle.gather(v, idx, m["W"], m["Hq"])) == lm["v_out_sha256"]


# C3 (H2O 8k, all 32 heads) — the one BASELINE config whose selection is not the reference's in every head.  Named, not
# thresholded: head 27, and in it ONE pooled score (key 28: the reference 0x3f72, the fmaf-chain product 0x3f73 — a column sum of
# 8 000 bf16 probabilities out of torch's opaque bf16 GEMM; the oracle's exactly-rounded-dot mode lands on the reference's
# side for this one and on neither side for six of the other nine scores that differ in the whole config).  Key 28 is not
# even selected: it sits in the first k elements, so it shapes the heap that later decides which of the 29 candidates tied at
# the k-th value survive — index 1251 (product) instead of 1700 (reference).
C3_RESIDUAL = {"head": 27, "score_index": 28, "reference_bits": 0x3f72, "product_bits": 0x3f73, "product_only": [1251], "reference_only": [1700]}


def test_c3_residual_is_one_score_bit_of_one_head(oracle):
    """The oracle on head 27 of C3: its scores differ from the reference's stored scores of that head in exactly one place, the
    top-k restatement on the REFERENCE's scores returns the reference's indices, and on its own scores the selection differs by
    exactly one index (tests/test_gpu_parity.py asserts the same of the GPU, and identity for the other 31 heads)."""
    m, arr = G.MANIFEST["C3_h2o_8k"], G.arrays("C3_h2o_8k")
    R = C3_RESIDUAL
    h = R["head"]
    q, k, v = G.inputs(m, expanded=False)
    g = m["Hq"] // m["Hkv"]
    sc = oracle.scores(q[:, h:h + 1].contiguous(), k[:, h // g:h // g + 1].contiguous(), m["W"], m["kernel"], "avgpool", full_rows=True,
                       **G.product_modes(oracle, m))
    ref_sc = G.from_bits(arr[f"scores_head{h}"], G.DT[m["dtype"]]).reshape(1, -1).contiguous()
    diff = (G.bits(sc).reshape(-1) != G.bits(ref_sc).reshape(-1)).nonzero().flatten().tolist()
    assert diff == [R["score_index"]]
    assert int(G.bits(ref_sc)[0, diff[0]]) & 0xffff == R["reference_bits"] and int(G.bits(sc).reshape(-1)[diff[0]]) & 0xffff == R["product_bits"]
    ref_idx = torch.from_numpy(arr["indices"])[h]
    idx_on_ref, _ = oracle.topk(ref_sc, m["n_keep"], oracle.TIES_TORCH)
    assert torch.equal(idx_on_ref[0], ref_idx)
    idx_own, _ = oracle.topk(sc.reshape(1, -1).contiguous(), m["n_keep"], oracle.TIES_TORCH)
    a, b = set(idx_own[0].tolist()), set(ref_idx.tolist())
    assert sorted(a - b) == R["product_only"] and sorted(b - a) == R["reference_only"]


@pytest.mark.parametrize("name", G.names(lambda m: m["method"] == "streamingllm" and not m["passthrough"]))
def test_streamingllm(oracle, name):
    """A11: first cap-W + last W tokens."""
    m = G.MANIFEST[name]
    q, k, v = _inputs(m)
    ko, vo, idx = oracle.streaming(k, v, m["W"], m["cap"] - m["W"], m["Hq"])
    assert list(ko.shape) == m["out_shape"]
    assert G.sha(ko) == m["k_out_sha256"] and G.sha(vo) == m["v_out_sha256"]


@pytest.mark.parametrize("name", G.names(lambda m: m["method"] == "pyramidkv"))
def test_pyramid_schedule(oracle, name):
    """A9: the per-layer budget equals the k the reference actually passed to topk (or pass-through)."""
    m = G.MANIFEST[name]
    k = oracle.pyramid_k(m["cap"], m["W"], m["L"], m["layer_idx"], m["n_layers"])
    assert k == (-1 if m["passthrough"] else m["n_keep"])


def test_pyramid_schedule_matches_survey_tables(oracle):
    ks = [oracle.pyramid_k(128, 8, 8000, l, 32) for l in range(32)]
    assert ks[0] == 234 and ks[31] == 17 and ks[0] - ks[1] == 7 and sum(ks) == 4016
    ks5 = [oracle.pyramid_k(2048, 8, 32000, l, 32) for l in range(32)]
    assert ks5[0] == 3978 and ks5[31] == 103 and ks5[0] - ks5[1] == 125 and sum(ks5) == 65296


def test_dtype_helpers(oracle):
    """fp16/bf16 conversions of the oracle == torch's (every fp16 bit pattern, and a sweep of fp32 values)."""
    L = oracle.lib()
    allh = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    f = allh.float()
    ok = ~torch.isnan(f)
    mine = torch.tensor([L.kvco_f16_to_f32(int(b) & 0xFFFF) for b in allh.view(torch.int16).tolist()])
    assert torch.equal(mine[ok], f[ok])
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(20000, generator=g) * s for s in (1e-8, 1e-5, 1e-3, 1.0, 300.0, 70000.0)])
    x = torch.cat([x, torch.tensor([0.0, -0.0, 65504.0, 65519.9, 65520.0, 1e-8, 5.96e-8, 2.98e-8, 6.1e-5, float("inf")])])
    th = x.to(torch.float16).view(torch.int16).to(torch.int32) & 0xFFFF
    tb = x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    assert th.tolist() == [L.kvco_f32_to_f16(float(v)) for v in x.tolist()]
    assert tb.tolist() == [L.kvco_f32_to_bf16(float(v)) for v in x.tolist()]


@pytest.mark.parametrize("name", G.names(lambda m: RAGGED(m) and not m["passthrough"] and m["L"] <= 1100))
def test_adakv_headkv_against_reference(oracle, name):
    """the oracle's restatement of AdaKVCluster / HeadKVCluster.update_kv (pyramidkv_utils.py:674-757, :813-878)
    against the imported reference's golden vectors: per-head lengths, the indices every head keeps (a prefix of torch-CPU's
    descending sort = libstdc++ std::sort, tie order included) and the flattened K / V byte for byte — every dtype.  (The two
    8k x 32-head fixtures are checked by the GPU suite, which also runs the oracle on them.)"""
    m, arr = G.MANIFEST[name], G.arrays(name)
    q, k, v = _inputs(m)
    g = m["Hq"] // m["Hkv"]
    kf, vf, lens, caps, idx, sc = oracle.ragged(q, k[:, ::g].contiguous(), v[:, ::g].contiguous(), m["W"], m["cap"], m["kernel"],
                                                m["pooling"], m.get("floor", 0.2), m.get("normalize", True), m.get("head_capacity"))
    ref_lens = torch.from_numpy(arr["head_lens"])
    assert torch.equal(lens, ref_lens)
    kept = torch.from_numpy(arr["kept_indices"])
    for h in range(m["Hq"]):
        c = int(ref_lens[h]) - m["W"]
        assert torch.equal(idx[h, :c], kept[h, :c])
    assert list(kf.shape) == m["out_shape"] and G.sha(kf) == m["k_out_sha256"] and G.sha(vf) == m["v_out_sha256"]
    ref_sc = G.from_bits(arr["scores"], G.DT[m["dtype"]])
    d = G.ulp_diff(sc, ref_sc)
    assert int(d.max()) <= (32 if m["dtype"] == "fp32" else 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", G.KILLERS)
def test_topk_on_adversarial_rows(oracle, name, dtype):
    """Rows built by McIlroy's adversary against the real libstdc++ nth_element + sort (oracle/killer_adversary.h): every
    partition is degenerate, introselect / introsort spend their depth budget and fall back to heap select / heap sort.
    The oracle must return what torch-CPU topk returned when the fixture was generated, and what it returns here."""
    sc, k, want = G.killer(name, dtype)
    got, _ = oracle.topk(sc, k, oracle.TIES_TORCH)
    assert torch.equal(got, want)
    assert torch.equal(torch.topk(sc.float(), k, dim=-1).indices, want)


L2N = lambda m: m["method"] == "l2norm"          # noqa: E731


@pytest.mark.parametrize("name", G.names(lambda m: L2N(m) and not m["passthrough"] and m["L"] <= 8000))
def test_l2norm_against_reference(oracle, name):
    """SURVEY 8f N4, L2NormCluster.update_kv (pyramidkv_utils.py:394-429): the oracle's norms (torch's 8-accumulator order),
    ascending std::sort and gather against what the imported reference produced — kept indices in order, norms bit for bit
    (small fixtures), SHA-256 of K' and V'.  fp32: torch fuses the multiply-add of its fp32 norm and the restatement does
    not (oracle/kvc_oracle.cpp), so fp32 fixtures compare the indices only where the norms agree."""
    m = G.MANIFEST[name]
    a = G.arrays(name)
    q, k, v = G.inputs(m)
    if m.get("coarse_k"):
        k = (k.float() * 2).round().div(2).to(k.dtype)
    ko, vo, idx, norms = oracle.l2norm(k, v, m["cap"], m["Hq"])
    if m["dtype"] != "fp32":
        if "norms" in a:
            assert torch.equal(G.bits(norms), torch.from_numpy(a["norms"]))
        assert torch.equal(idx, torch.from_numpy(a["indices"]))
        assert G.sha(ko) == m["k_out_sha256"] and G.sha(vo) == m["v_out_sha256"]
    else:
        same = (G.bits(norms) == torch.from_numpy(a["norms"])).all(dim=1)
        assert int(same.sum()) >= 1 or m["Hq"] <= 8
        want = torch.from_numpy(a["indices"])
        for h in range(m["Hq"]):
            if bool(same[h]):
                assert torch.equal(idx[h], want[h])


@pytest.mark.parametrize("name", G.names(lambda m: m["method"].startswith("merge_")))
def test_merge_pivot_against_reference(oracle, name):
    """SURVEY 8f N4, merge_kv(..., "pivot") (pyramidkv_utils.py:119-170): the oracle's restatement fed the reference's own topk
    indices — number of dropped tokens, the pivot of every dropped token (captured at the reference's similarity.max), and the
    merged K / V bit for bit (SHA-256), at 8k -> 128 with 32 heads too (159 168 pivots)."""
    m = G.MANIFEST[name]
    a = G.arrays(name)
    q, k, v = G.inputs(m)
    ko, vo, piv = oracle.merge_pivot(k, v, torch.from_numpy(a["indices"]).contiguous(), m["W"])
    assert piv.shape[1] == m["drop_len"]
    assert torch.equal(piv, torch.from_numpy(a["pivot"].astype("int32")))
    assert G.sha(ko) == m["k_out_sha256"] and G.sha(vo) == m["v_out_sha256"]


@pytest.mark.parametrize("name", G.names(lambda m: m["method"] == "think" and not m["passthrough"]))
def test_think_prune_against_reference(oracle, name):
    """SURVEY 8f N4, key_pruner_query_driven (pyramidkv_utils.py:13-26) on the keys compressed with the reference's own topk indices:
    channel scores bit for bit (captured at the reference's topk(largest=False)), the channel mask, and the pruned / recent keys
    (SHA-256) — every dtype, 8k -> 128 and 8k -> 2048 included."""
    m = G.MANIFEST[name]
    a = G.arrays(name)
    q, k, v = G.inputs(m)
    kc = oracle.gather(k, torch.from_numpy(a["indices"]).contiguous(), m["W"], m["Hq"])
    pruned, recent, keep, sc = oracle.think_prune(kc, q, m["recent"], m["ratio"])
    assert torch.equal(G.bits(sc), torch.from_numpy(a["channel_scores"]))
    assert torch.equal(keep[0], torch.from_numpy(a["keep"]).bool())
    assert G.sha(pruned) == m["pruned_sha256"] and G.sha(recent.contiguous()) == m["recent_sha256"]


@pytest.mark.parametrize("name", G.names(lambda m: m["method"] == "cam" and not m["passthrough"]))
def test_cam_given_the_references_draws(oracle, name):
    """SURVEY 8f N4, CAM (pyramidkv_utils.py:431-513) split at its random draw: the oracle's window-sum scores and every token's
    merge probability against what the reference handed to its .topk and to torch.bernoulli (bf16 / fp16: within the flip budget
    of the other scored fixtures — at most max(2, 0.5 %) entries off by one unit in the last place; fp32: a few ulp, torch's
    softmax exp is opaque); then, GIVEN the reference's recorded draws, the in-place value merge (SHA-256 of the mutated
    value_states: exact in every dtype), the top-k on the reference's scores and the gathered K' / V' — bit for bit."""
    m, arr = G.MANIFEST[name], G.arrays(name)
    q, k, v = _inputs(m)
    dt = G.DT[m["dtype"]]
    sc, prob = oracle.cam_plan(q, k, m["W"], m["start_budget"], **G.product_modes(oracle, m))
    ref_prob = G.from_bits(arr["prob"], dt)
    mask = torch.from_numpy(arr["mask"])
    d = G.ulp_diff(prob, ref_prob)
    if m["dtype"] == "fp32":
        assert int(d.max()) <= 64
    else:
        assert int(d.max()) <= 1 and int((d > 0).sum()) <= max(2, d.numel() // 200)
        if "scores" in arr:
            ds = G.ulp_diff(sc, G.from_bits(arr["scores"], dt))
            assert int(ds.max()) <= 1 and int((ds > 0).sum()) <= max(2, ds.numel() // 200)
    merged = oracle.cam_merge(v, mask, m["W"], m["start_budget"])
    assert G.sha(merged) == m["merged_values_sha256"]                    # the recurrence is exact given the draws
    ref_idx = torch.from_numpy(arr["indices"])
    if "scores" in arr:                                                   # the selection on the reference's own scores
        idx, _ = oracle.topk(G.from_bits(arr["scores"], dt).contiguous(), m["n_keep"], oracle.TIES_TORCH)
        assert torch.equal(idx, ref_idx)
    assert G.sha(oracle.gather(k, ref_idx, m["W"], m["Hq"])) == m["k_out_sha256"]
    assert G.sha(oracle.gather(merged, ref_idx, m["W"], m["Hq"])) == m["v_out_sha256"]
    if G.sha(sc) == m["scores_sha256"]:                                   # scores identical: the whole update_kv is
        ko, vo, idx, _, _, _ = oracle.cam(q, k, v, m["W"], m["n_keep"], m["start_budget"], mask, **G.product_modes(oracle, m))
        assert torch.equal(idx, ref_idx) and G.sha(ko) == m["k_out_sha256"] and G.sha(vo) == m["v_out_sha256"]
    else:
        assert m["dtype"] != "bf16", "every bf16 CAM fixture reproduces the reference's scores bit for bit"
