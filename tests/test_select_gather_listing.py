"""Build check of select_gather_kernel (the exact selection + K / V gather in one workgroup of two waves).

Past the barrier at entry its two waves follow different control flow, so the kernel may hold exactly ONE s_barrier: a
second one would wait for a wave that never arrives.  The heap wave runs WaveHeapL's hand-scheduled step blocks, which
are copied verbatim from the source; the copy wave's rows stay in registers (no scratch).  Checked in the gfx950 listing
(hipcc -S cross-compiles without a GPU).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kvcache_factory_amd", "csrc")


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-C", CSRC, "-s", os.path.join("isa", "kvc_select_exact.s")], stderr=subprocess.DEVNULL)
    return open(os.path.join(CSRC, "isa", "kvc_select_exact.s")).read()


def _body(text, kernel):
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(kernel), text, re.S | re.M)
    assert m, kernel
    return m.group(1)


def _meta(text, kernel, key):
    m = re.search(r"\.name:\s+%s\n(?:(?!\.name:).)*?\.%s:\s+(\d+)" % (re.escape(kernel), key), text, re.S)
    assert m, (kernel, key)
    return int(m.group(1))


@pytest.mark.parametrize("dt", [0, 1])                  # KVC_BF16, KVC_FP16
def test_select_gather_kernel_listing(listing, dt):
    fused = "_ZN3kvc20select_gather_kernelILi%dEEEvNS_10SelectArgsE" % dt
    alone = "_ZN3kvc19select_exact_kernelILi%dEEEvNS_10SelectArgsEPyii" % dt
    body = _body(listing, fused)
    assert len(re.findall(r"^\s*s_barrier\b", body, re.M)) == 1
    assert _meta(listing, fused, "private_segment_fixed_size") == 0
    assert _meta(listing, fused, "vgpr_spill_count") == 0 and _meta(listing, fused, "sgpr_spill_count") == 0
    # the heap step's hand-scheduled blocks keep their hazard spacing (an instruction between a VALU-written SGPR mask and
    # the VALU instruction that reads it: DESIGN.md §3)
    step = re.compile(r"v_cmp_gt_u32_sdwa (s\[\d+:\d+\]), v\d+, v\d+ src0_sel:WORD_1 src1_sel:WORD_1\n\s*v_cndmask_b32_e64 v\d+, v\d+, v\d+, \1")
    assert not step.search(body), "a VALU read of a VALU-written mask right behind its compare (gfx950 VALUWriteSGPRVALURead)"
    assert "v_cmp_gt_u32_sdwa vcc" in body and "v_cmp_gt_u32_sdwa vcc" in _body(listing, alone)
