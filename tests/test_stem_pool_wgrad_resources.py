"""Compile-time resources of stem_wgrad_pool_kernel (csrc/conv/stem_halo.hip) for
gfx950: no scratch, LDS within the 160 KB of a CU, one 256-thread block per CU
(one wave per SIMD, the whole 512-register budget) as designed."""
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                                reason="needs hipcc and c++filt")


def test_stem_wgrad_pool_kernel_resources():
    from tools.kernel_resources import resources
    ks = [k for k in resources(os.path.join(ROOT, "csrc/conv/stem_halo.hip")) if "stem_wgrad_pool_kernel" in k["name"]]
    assert len(ks) == 2, [k["name"] for k in ks]  # pool pad 0 and pad 1
    for k in ks:
        assert k["scratch"] == "0", k
        assert int(k["lds"]) <= 163840, k
        assert int(k["lds"]) > 81920, k        # more than half a CU's LDS: one block per CU
        assert k["occupancy"] == "1", k
        assert int(k["vgpr"]) + int(k["agpr"]) <= 512, k
