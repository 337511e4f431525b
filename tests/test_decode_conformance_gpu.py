"""Decode-step conformance on the MI355X: both input families of tests/decode_ref.py through `_kvc` for all six entries, over the
grid test_decode_conformance_cpu.py has already run through the CPU stand-ins (so no input here can miss the needle condition).

Family A: the output is the needle's V row bit for bit on the unquantized entries (within 1 ulp of the dtype over a de-quantized
row), for every probe of every call; the scored step's scores move by exactly one row; appended rows are byte-identical and no
other buffer changes.  Family B: every output element within  1/2 ulp + 4 e_ref sum p |v|  of fp64; the measured e_kernel / e_ref is
printed per case and, as the largest per entry and dtype, by the last test (DESIGN.md section 4 records them)."""
import collections

import pytest
import torch

import decode_ref as R
from test_decode_conformance_cpu import run_bound, run_needles

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)
IDS = [R.spec_id(s) for s in R.GRID]


def entry_fn(kvc, spec):
    return {"step2": kvc.decode_step, "think": kvc.decode_step, "rows": kvc.decode_step_rows, "scored": kvc.decode_step_scored,
            "quant": kvc.decode_step_quant, "outl": kvc.decode_step_quant_outliers, "ragged": kvc.ragged_decode_step}[spec["entry"]]


@pytest.mark.parametrize("spec", R.GRID, ids=IDS)
def test_needles_row_exact(kvc, gpu_device, spec):
    probes = run_needles(spec, entry_fn(kvc, spec), gpu_device)
    print(f"{R.spec_id(spec)}: {probes} needles returned their row")


@pytest.mark.parametrize("spec", R.GRID, ids=IDS)
def test_per_element_bound(kvc, gpu_device, spec):
    e_kernel, e_ref = run_bound(spec, entry_fn(kvc, spec), gpu_device)
    key = (spec["entry"], str(spec["dtype"])[6:])
    RATIOS[key] = max(RATIOS[key], e_kernel / e_ref)
    print(f"{R.spec_id(spec)}: e_kernel / e_ref = {e_kernel / e_ref:.3f} (e_ref = {e_ref:.3e})")


def test_report_ratios():
    """The largest e_kernel / e_ref per entry and dtype of this run (the bound allows 4)."""
    for (entry, dt), r in sorted(RATIOS.items()):
        print(f"e_kernel / e_ref  {entry:7s} {dt:9s} {r:.3f}")
        assert r <= R.FACTOR
