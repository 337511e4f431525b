"""Build audit of the K scan's prefetch (kvc_score.hip: logits_kernel).  The next tile's global loads are issued ahead of
the MFMA chain so that they are in flight during it; their only wait is commit()'s, after the chain.  Whether that holds
is decided by the compiler: with a ragged (zero-filling, predicated) arm inside issue() hipcc merged both arms into a
shared tail that carried `s_waitcnt vmcnt(0)` — every wave waited a whole HBM round trip for the loads it had just
issued before its first MFMA of every tile.  tools/asm_audit.py: pipeline_stats() walks the full-tile path of the tile
loop in the listing; this test requires it free of vmcnt waits for every instantiation, in both dot modes, and holds
the VALU instructions on that path at or below what they were before the loads took an SGPR base.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_audit  # noqa: E402

CSRC = os.path.join(ROOT, "kvcache_factory_amd", "csrc")

# VALU instructions from the first next-tile load to the last MFMA, full-tile path, before this audit existed
# (one 64-bit address add per load and a zero fill; the exact fp16 / fp32 scans convert their B operands on the VALU).
# Keyed by (dtype, D, mfma16); the runtime-W instantiations had the same or two more.
VALU_BEFORE = {(0, 128, 0): 9, (0, 128, 1): 9, (0, 64, 0): 5, (0, 64, 1): 5, (1, 128, 1): 9, (1, 64, 1): 5,
               (1, 128, 0): 137, (1, 64, 0): 69, (2, 128, 0): 81, (2, 64, 0): 41}
LOOP_VALU_BEFORE_HEADLINE = 661              # logits_kernel<bf16, 128, 8, exact>: whole loop body, every arm


@pytest.fixture(scope="module")
def logits_kernels():
    subprocess.check_call(["make", "-C", CSRC, "-s", os.path.join("isa", "kvc_score.s")], stderr=subprocess.DEVNULL)
    res = asm_audit.audit_file(os.path.join(CSRC, "isa", "kvc_score.s"), ("logits_kernel",))
    out = {}
    for name, (_, stats) in res.items():
        m = re.search(r"logits_kernelILi(\d)ELi(\d+)ELi(\d+)ELb([01])E", name)
        assert m, name
        out[tuple(int(x) for x in m.groups())] = stats
    return out


def test_every_instantiation_is_there(logits_kernels):
    """bf16 / fp16 in both dot modes, fp32 exact only; D in {64, 128}; W in {8, 16, 32, 64, runtime}."""
    want = {(dt, d, w, f) for dt in (0, 1, 2) for d in (64, 128) for w in (0, 8, 16, 32, 64) for f in (0, 1) if not (dt == 2 and f)}
    assert set(logits_kernels) == want


def test_next_tile_loads_stay_in_flight_across_the_chain(logits_kernels):
    for key, stats in sorted(logits_kernels.items()):
        p = stats["pipeline"]
        dt, d = key[0], key[1]
        assert p is not None and p["path_complete"], key
        assert p["path_loads"] == d * (4 if dt == 2 else 2) // 32, (key, p)       # every load of the tile is ahead of the chain
        assert p["vm_waits"] == [], (key, p)


def test_valu_on_the_path_is_no_higher_than_before(logits_kernels):
    for (dt, d, w, f), stats in sorted(logits_kernels.items()):
        p = stats["pipeline"]
        print((dt, d, w, f), "path_valu", p["path_valu"], "loop_valu", p["loop_valu"])
        assert p["path_valu"] <= VALU_BEFORE[(dt, d, f)], ((dt, d, w, f), p)
    assert logits_kernels[(0, 128, 8, 0)]["pipeline"]["loop_valu"] <= LOOP_VALU_BEFORE_HEADLINE


def _listing(shared_tail_wait):
    """A tile loop in the shape hipcc gave the two-armed issue(): the full-tile arm issues its loads and jumps to a tail it
    shares with the ragged arm; the tail loads the last chunk and the chain follows."""
    wait = ["\ts_waitcnt vmcnt(0)"] if shared_tail_wait else []
    return [".LBB1_35:",
            "\ts_cbranch_scc1 .LBB1_38",
            "\tv_lshl_add_u64 v[2:3], s[42:43], 0, v[64:65]",
            "\tglobal_load_dwordx4 v[18:21], v[2:3], off",
            "\tglobal_load_dwordx4 v[22:25], v[2:3], off",
            "\ts_cbranch_execz .LBB1_39",
            "\ts_branch .LBB1_54",
            ".LBB1_38:",
            "\tv_mov_b32_e32 v18, 0",
            ".LBB1_39:",
            "\ts_waitcnt vmcnt(1)",                          # the ragged arm: not on the full-tile path
            "\tglobal_load_dwordx4 v[18:21], v[4:5], off",
            ".LBB1_54:",
            *wait,
            "\tv_mov_b32_e32 v46, 0",
            "\tglobal_load_dwordx4 v[46:49], v[2:3], off",
            "\tv_mfma_f32_32x32x2_f32 v[2:17], v1, v5, v[2:17]",
            "\tv_mfma_f32_32x32x2_f32 v[2:17], v1, v6, v[2:17]",
            "\ts_waitcnt vmcnt(0)",                          # commit's wait, after the chain
            "\tds_write_b128 v9, v[18:21]",
            "\ts_cbranch_vccnz .LBB1_35",
            ".Lfunc_end1:"]


def test_rule_on_synthetic_listings():
    bad = asm_audit.pipeline_stats(_listing(True))
    assert bad["path_complete"] and bad["path_loads"] == 3 and bad["path_valu"] == 1
    assert len(bad["vm_waits"]) == 1                        # the shared tail's wait, and only that one
    good = asm_audit.pipeline_stats(_listing(False))
    assert good["path_complete"] and good["path_loads"] == 3 and good["vm_waits"] == []
    assert asm_audit.pipeline_stats(["\tv_mov_b32_e32 v1, 0", ".Lfunc_end0:"]) is None     # no MFMA loop at all
