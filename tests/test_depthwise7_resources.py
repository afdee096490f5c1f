"""Build-time guard for the depthwise kernels.  7x7 (csrc/conv/depthwise7.hip):
every instantiation builds for gfx950 without scratch -- the design keeps 98
weight registers and a tile of accumulators live, and a spill is a silent
2-4x -- at two waves per SIMD; only the weight gradient uses LDS (its 2 x 256
fp32 lane-combine buffer) beside the fp64 fold of the shared column reduce
(csrc/conv/dw_common.h).  3x3 (csrc/conv/depthwise.hip): every instantiation
without scratch -- a runtime stride once indexed the tap registers dynamically
and cost 2-4x through scratch.  CPU only (hipcc cross-compiles gfx950)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                                 reason="needs hipcc and c++filt")


def _kernels(name):
    from tools.kernel_resources import resources  # (c++filt leaves the bf16 names mangled: match by substring)
    return resources(os.path.join(ROOT, "csrc", "conv", name))


@needs_hipcc
def test_depthwise7_kernels_build_without_scratch():
    ks = _kernels("depthwise7.hip")
    conv = [k for k in ks if "dw7_kernel" in k["name"]]
    wgrad = [k for k in ks if "dw7_wgrad_kernel" in k["name"]]
    red = [k for k in ks if "dw_colreduce_kernel" in k["name"]]
    # forward / dgrad x bf16 / fp32 weights; one weight gradient; the reduce in bf16 / fp32
    assert (len(conv), len(wgrad), len(red), len(ks)) == (4, 1, 2, 7), [k["name"] for k in ks]
    bad = [(k["name"], k["scratch"]) for k in ks if k["scratch"] != "0"]
    assert not bad, bad
    assert all(int(k["lds"]) == 0 for k in conv), [(k["name"], k["lds"]) for k in conv]
    assert int(wgrad[0]["lds"]) == 2 * 256 * 4
    assert all(int(k["lds"]) == 1024 * 8 for k in red)
    # 256 registers or fewer (no AGPR copies): two waves per SIMD
    for k in conv + wgrad:
        assert int(k["vgpr"]) <= 256 and int(k["agpr"]) == 0 and int(k["occupancy"]) >= 2, k


@needs_hipcc
def test_depthwise3_kernels_build_without_scratch():
    ks = _kernels("depthwise.hip")
    # forward: 2 activation x 2 weight dtypes x moments x stride; data gradient: the same without
    # moments; weight gradient: activation dtype x stride; the reduce in bf16 / fp32
    count = [sum(n in k["name"] for k in ks) for n in ("dw_fwd_kernel", "dw_dgrad_kernel", "dw_wgrad_kernel",
                                                       "dw_colreduce_kernel")]
    assert (count, len(ks)) == ([16, 8, 4, 2], 30), [k["name"] for k in ks]
    bad = [(k["name"], k["scratch"]) for k in ks if k["scratch"] != "0"]
    assert not bad, bad
