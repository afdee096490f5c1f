"""Compile-time resources of bn_apply_gram_kernel (csrc/bn/bn_apply_gram.hip) for
gfx950.  Its C = 256 instantiations hold the Gram accumulators in AGPRs behind
inline-asm MFMAs (w4_mfma), so a compiler spill of one would read a value still
being written: every instantiation must build with zero scratch, and the
occupancy each width's grid was sized for must hold (4 / 2 / 1 waves per SIMD
at C = 64 / 128 / 256)."""
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                                reason="needs hipcc and c++filt")


def test_bn_apply_gram_kernel_resources():
    from tools.kernel_resources import resources
    ks = [k for k in resources(os.path.join(ROOT, "csrc/bn/bn_apply_gram.hip")) if "bn_apply_gram_kernel" in k["name"]]
    assert len(ks) == 6, [k["name"] for k in ks]  # C = 64, 128, 256 x streaming or not
    want = {64: (4, 16384), 128: (2, 32768), 256: (1, 65536)}
    seen = set()
    for k in ks:
        # demangled, or still mangled where c++filt does not know the bf16 type
        c = int(re.search(r"bn_apply_gram_kernel(?:<\s*|ILi)(\d+)", k["name"]).group(1))
        seen.add(c)
        occ, lds = want[c]
        assert k["scratch"] == "0", k
        assert int(k["lds"]) == lds, k
        assert int(k["occupancy"]) >= occ, k
        assert int(k["vgpr"]) + int(k["agpr"]) <= 512 // occ, k
        if c == 256:
            assert int(k["agpr"]) == 256, k
    assert seen == {64, 128, 256}
