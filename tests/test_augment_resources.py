"""Build-time guard for the augmentation kernel (csrc/data/augment.hip): every
instantiation (fp32 / bf16, channels-last / NCHW, crop-only / with resize, vector / scalar) builds for
gfx950 without scratch, and its LDS is the normalisation table alone (4 channels
x 256 fp32 entries).  CPU only (hipcc cross-compiles gfx950)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
def test_augment_kernels_build_without_scratch():
    from tools.kernel_resources import resources  # (c++filt leaves the bf16 names mangled: match by substring)
    ks = [k for k in resources(os.path.join(ROOT, "csrc", "data", "augment.hip")) if "augment_kernel" in k["name"]]
    assert len(ks) == 16, [k["name"] for k in ks]
    bad = [(k["name"], k["scratch"]) for k in ks if k["scratch"] != "0"]
    assert not bad, bad
    assert all(0 < int(k["lds"]) <= 4 * 256 * 4 for k in ks), [(k["name"], k["lds"]) for k in ks]
