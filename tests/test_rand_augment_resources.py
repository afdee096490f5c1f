"""Build-time guard for the RandAugment kernels (csrc/data/rand_augment.hip): the byte crop, the
histogram pass and every instantiation of the apply pass (the two staging ones; last slot: fp32 / bf16,
channels-last / NCHW, vector / scalar) build for gfx950 without scratch, and their LDS is no more than
the sum the file documents: histograms 4 x 256 x 4 + byte tables 3 x 256 + normalisation table
3 x 256 x 4.  CPU only (hipcc cross-compiles gfx950)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIST_LDS = 4 * 256 * 4
APPLY_LDS = HIST_LDS + 3 * 256 + 3 * 256 * 4


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
def test_rand_augment_kernels_build_without_scratch():
    from tools.kernel_resources import resources  # (c++filt leaves the bf16 names mangled: match by substring)
    src = os.path.join(ROOT, "csrc", "data", "rand_augment.hip")
    assert f"= {APPLY_LDS} bytes" in open(src).read()  # the documented sum
    ks = resources(src)
    by = {tag: [k for k in ks if tag in k["name"]] for tag in ("crop_bytes_kernel", "rand_hist_kernel", "rand_apply_kernel")}
    assert sum(len(v) for v in by.values()) == len(ks), [k["name"] for k in ks]
    assert len(by["crop_bytes_kernel"]) == 1 and len(by["rand_hist_kernel"]) == 1
    assert len(by["rand_apply_kernel"]) == 10, [k["name"] for k in by["rand_apply_kernel"]]
    bad = [(k["name"], k["scratch"]) for k in ks if k["scratch"] != "0"]
    assert not bad, bad
    assert int(by["crop_bytes_kernel"][0]["lds"]) == 0
    assert int(by["rand_hist_kernel"][0]["lds"]) == HIST_LDS
    lds = sorted(int(k["lds"]) for k in by["rand_apply_kernel"])
    assert lds == [APPLY_LDS - 3 * 256 * 4] * 2 + [APPLY_LDS] * 8, lds
