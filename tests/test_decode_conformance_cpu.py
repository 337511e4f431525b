"""The decode-step conformance harness (tests/decode_ref.py) judged without a GPU: the suite's correct CPU stand-ins of the six
entries pass both input families over the whole grid of the GPU file with no probe left out (which also proves the needle
condition for every shape the GPU will meet), deliberately wrong restatements are rejected, and the old absolute bound's blind
spot is on record."""
import numpy as np
import pytest
import torch

import cpu_compress
import decode_ref as R
import heavy_hitter_ref
import kvquant_ref
import quant_ref
from test_batch_generation_cpu import restated_decode_step_rows

STANDINS = dict(step2=cpu_compress.oracle_decode_step, think=cpu_compress.oracle_decode_step, rows=restated_decode_step_rows,
                scored=heavy_hitter_ref.standin_decode_step_scored, quant=quant_ref.decode_step_quant,
                outl=kvquant_ref.decode_step_quant_outliers, ragged=R.standin_ragged_decode_step)


def run_needles(spec, fn, device=None, seed=11):
    """Every needle call of a spec through fn: the condition for every probe, the needles, the scores, the buffers.  -> probes checked."""
    done = 0
    for case in R.needle_calls(spec, seed):
        case.check_condition()                                              # ProbeInputError: the inputs are wrong, nothing is skipped
        out, after = case.run(fn, device)
        done += case.check_needles(out)
        if case.entry == "scored":
            case.check_scores(after)
        case.check_buffers(after)
    return done


def run_bound(spec, fn, device=None, seed=5):
    case = R.Case(spec, "B", seed)
    out, after = case.run(fn, device)
    case.check_buffers(after)
    return case.check_bound(out)


@pytest.mark.parametrize("spec", R.GRID, ids=[R.spec_id(s) for s in R.GRID])
def test_standins_pass_both_families(spec):
    probes = run_needles(spec, STANDINS[spec["entry"]])
    rows = spec.get("P1", 0) + int(np.max(spec["P"])) + spec.get("Tq", 0) + spec.get("T", 0) + spec["t"]
    assert probes >= (rows if rows <= 320 else rows // 16)                  # every row of a small cache, two in 32 of a large one
    e_kernel, e_ref = run_bound(spec, STANDINS[spec["entry"]])
    assert e_kernel <= R.FACTOR * e_ref


def test_grid_covers_every_instantiation():
    """3 dtypes x 2 head dims per kernel (x 3 code widths for the quantized ones), without and with splits where the kernel has both;
    the cap of 64 splits; every code width x group size; a transposed query and t in {1, 3, 5} per entry."""
    for e in R.ENTRIES:
        specs = [s for s in R.GRID if s["entry"] == e]
        assert {s["t"] for s in specs} == {1, 3, 5} and any(s.get("q_view") and s["t"] > 1 for s in specs), e
        for dt, D in R.COMBOS:
            mine = [s for s in specs if s["dtype"] == dt and s["D"] == D]
            assert {R.splits_of(s) > 1 for s in mine} == ({False} if e == "ragged" else {False, True}), (e, dt, D)
            if e in R.QUANTIZED:
                assert {s["nbits"] for s in mine} == {2, 4, 8}
        if e in R.QUANTIZED:
            assert {(s["nbits"], s["G"]) for s in specs} == {(nb, G) for nb in (2, 4, 8) for G in (32, 64, 128)}
            assert {s["b"] for s in specs} == {1, 2} and any(s["T"] == 0 for s in specs) and any(s["T"] == s["R"] - 1 for s in specs)
            assert any(s["Tq"] == 0 for s in specs) and any(s["Tq"] == s["G"] for s in specs) and any(s["Tq"] > s["G"] for s in specs)
            assert all(s["P"] % s["G"] for s in specs)                      # a partial last key group in every prefix
    assert any(R.splits_of(s) == 64 for s in R.GRID)
    assert any(s["hq"] * s["t"] <= 16 and s.get("b", 1) == 1 and s["P"] + s["T"] + s["t"] >= 4160 for s in R.GRID if s["entry"] == "step2")
    assert {s["b"] for s in R.GRID if s["entry"] == "step2"} == {1, 2}
    assert any(s["entry"] == "rows" and s["P"][:5] == [0, 1, 63, 64, 65] for s in R.GRID)
    assert any(s.get("v_outliers") for s in R.GRID)


def _mutant_specs():
    """Per entry one spec without splits and one with (t > 1, so the causal mutant applies)."""
    out = []
    for e in R.ENTRIES:
        for split in (False, True):
            mine = [s for s in R.GRID if s["entry"] == e and s["t"] > 1 and (R.splits_of(s) > 1) == split and
                    (e != "step2" or s["hkv"] not in (1, s["hq"]))]          # step2: a GQA group, so the KV-head mutant applies
            if mine:
                out.append(min(mine, key=lambda s: (s.get("P1", 0) + int(np.max(s["P"]))) * s["hq"] * s.get("b", 1)))
    return out


MUTANT_SPECS = _mutant_specs()
# Family B's verdicts, on record: what the numerical check alone sees of each wrong restatement on these cases.
B_ALWAYS_REJECTS = ("double_count", "see_extra_new_row", "tail_wrong_kv_head", "v_shift_in_block", "skip_outlier_patch_k")


@pytest.mark.parametrize("spec", MUTANT_SPECS, ids=[R.spec_id(s) for s in MUTANT_SPECS])
def test_wrong_restatements_are_rejected(spec):
    """Every mutant that applies to the case is rejected by the needles, except the row counted twice: a needle counted twice
    still returns its own V, so that one is family B's to reject."""
    calls = R.needle_calls(spec, 11)
    for c in calls:
        c.check_condition()
    caseb = R.Case(spec, "B", 5)
    applied = [m for m in R.MUTANTS if R.mutant_applies(calls[0], m)]
    assert {"drop_segment_last", "double_count", "v_shift_in_block", "see_extra_new_row"} <= set(applied)
    verdict_b = {}
    for m in applied:
        missed = 0
        for c in calls:
            try:
                c.check_needles(R.mutant_out(c, m))
            except AssertionError:
                missed += 1
        try:
            caseb.check_bound(R.mutant_out(caseb, m))
            verdict_b[m] = False
        except AssertionError:
            verdict_b[m] = True
        if m == "double_count":
            assert missed == 0 and verdict_b[m], m
            if spec["entry"] == "scored":                                   # and the scored step's: the needle's score grows by 1/2
                hit = [c for c in calls if any(r % 64 == 0 for _, _, _, r in c.probes)]
                assert hit
                for c in hit:
                    with pytest.raises(AssertionError):
                        c.check_scores(R.mutant_scores_double_count(c))
        else:
            assert missed > 0, f"the needles accept the mutant {m}"
    print("family B rejects:", verdict_b)
    for m in B_ALWAYS_REJECTS:
        assert verdict_b.get(m, True), m


def test_every_mutant_is_applied_somewhere():
    seen = set()
    for spec in MUTANT_SPECS:
        c = R.Case(spec, "B", 5)
        seen |= {m for m in R.MUTANTS if R.mutant_applies(c, m)}
    assert seen == set(R.MUTANTS)


def test_old_bound_blind_spot():
    """The inputs of test_decode_step_vs_reference_shaped_attention at P = 2056, T = 300 (bf16, unit-variance data, same seed) with
    the last prefix row dropped: inside the old rule max |out - ref| <= 2^-7 max(1, max |ref|), outside the per-element bound."""
    dtype, D, hq, hkv, P, T, t = torch.bfloat16, 128, 32, 8, 2056, 300, 1
    g = torch.Generator().manual_seed(P + T)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dtype).float()      # noqa: E731
    q, kn, vn = rn(1, hq, t, D), rn(1, hkv, t, D), rn(1, hkv, t, D)
    kp, vp = rn(1, hq, P + 7, D), rn(1, hq, P + 7, D)
    kt, vt = rn(1, hkv, T + t + 4, D), rn(1, hkv, T + t + 4, D)
    c = R.Case(dict(entry="step2", dtype=dtype, D=D, hq=hq, hkv=hkv, t=t, P=P, T=T), "B", 0)
    c.q, c.nk, c.nv, c.ek, c.ev, c.tk, c.tv = q, kn, vn, kp, vp, kt[:, :, :T], vt[:, :, :T]
    c._finalize()
    c._assemble()
    ref, _ = c.ref64()
    honest = R._np64(torch.from_numpy(c.ref32()).to(dtype))
    keep = np.arange(P + T + t) != P - 1
    wrong, _ = R.attention64(R._np64(q), c.K[:, :, keep], c.V[:, :, keep], c.n - 1, c.scaling)
    wrong = R._np64(torch.from_numpy(wrong).to(dtype))
    old = lambda out: float(np.abs(out - ref).max()) <= 2.0 ** -7 * max(1.0, float(np.abs(ref).max()))      # noqa: E731
    assert old(honest) and old(wrong)                                       # the old rule cannot tell them apart
    c.check_bound(honest)
    with pytest.raises(AssertionError):
        c.check_bound(wrong)
