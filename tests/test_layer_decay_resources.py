"""adamw_scaled_kernel of csrc/optim/fused_adamw.hip compiles to the sixteen
instantiations the host launches, none of which spills."""
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
def test_scaled_step_kernel_instantiations_build_without_scratch():
    """(G, P) x MASTER x EMA, as adamw_flat_kernel: the host instantiates all 16."""
    import sys
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import resources
    ks = [k for k in resources(os.path.join(ROOT, "csrc/optim", "fused_adamw.hip"))
          if "adamw_scaled_kernel" in k["name"]]
    assert len(ks) == 16, [k["name"] for k in ks]
    assert not any("adamw_flat_kernel" in k["name"] for k in ks)
    for k in ks:
        print(k)
        assert k["scratch"] == "0", k
