"""Build-time guard for the random-erasing kernels (csrc/data/random_erase.hip): every instantiation
of the eraser (fp32 / bf16, channels-last / NCHW) and the philox_bits kernel build for gfx950 with no
scratch and no LDS, and the file holds as many kernels as it documents.  CPU only (hipcc
cross-compiles gfx950)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
def test_random_erase_kernels_build_without_scratch_and_lds():
    from tools.kernel_resources import resources  # (c++filt leaves the bf16 names mangled: match by substring)
    src = os.path.join(ROOT, "csrc", "data", "random_erase.hip")
    assert "= 4, and philox_bits_kernel = 5 kernels" in open(src).read()  # the documented count
    ks = resources(src)
    by = {tag: [k for k in ks if tag in k["name"]] for tag in ("random_erase_kernel", "philox_bits_kernel")}
    assert sum(len(v) for v in by.values()) == len(ks) == 5, [k["name"] for k in ks]
    assert len(by["random_erase_kernel"]) == 4 and len(by["philox_bits_kernel"]) == 1
    bad = [(k["name"], k["scratch"], k["lds"]) for k in ks if k["scratch"] != "0" or int(k["lds"]) != 0]
    assert not bad, bad
