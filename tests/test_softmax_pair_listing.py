"""Build check of softmax_pool_pair_kernel (the window-8 softmax stage with two heads per CU).

The kernel's point is its register footprint: two of its workgroups must be resident on one CU, with nothing in scratch.  A CU
has four SIMDs of 512 VGPRs per lane, allocated in granules of 8, and holds at most 32 waves.  Checked in the gfx950 listing's
kernel metadata (hipcc -S cross-compiles without a GPU): resource numbers only.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kvcache_factory_amd", "csrc")
THREADS = 1024                                              # the geometry launch_softmax_pool_t launches


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-C", CSRC, "-s", os.path.join("isa", "kvc_score.s")], stderr=subprocess.DEVNULL)
    return open(os.path.join(CSRC, "isa", "kvc_score.s")).read()


def _meta(text, kernel, key):
    m = re.search(r"\.name:\s+%s\n(?:(?!\.name:).)*?\.%s:\s+(\d+)" % (re.escape(kernel), key), text, re.S)
    assert m, (kernel, key)
    return int(m.group(1))


@pytest.mark.parametrize("dt", [0, 1])                  # KVC_BF16, KVC_FP16
def test_two_workgroups_fit_a_cu(listing, dt):
    kernel = "_ZN3kvc24softmax_pool_pair_kernelILi%dELi%dEEEvNS_9ScoreArgsE" % (dt, THREADS)
    assert _meta(listing, kernel, "private_segment_fixed_size") == 0
    assert _meta(listing, kernel, "vgpr_spill_count") == 0 and _meta(listing, kernel, "sgpr_spill_count") == 0
    assert _meta(listing, kernel, "max_flat_workgroup_size") == THREADS
    regs = _meta(listing, kernel, "vgpr_count") + _meta(listing, kernel, "agpr_count")
    alloc = -(-regs // 8) * 8
    w = THREADS // 64 // 4                                  # waves of one workgroup on each SIMD
    assert 2 * w * alloc <= 512, (regs, alloc)
    assert 2 * 4 * w <= 32
