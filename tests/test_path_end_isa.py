"""The static ISA audit still builds the bench module (no GPU): scripts/
jit_isa.py compiles the C2 scene's rt0_jit_pass with hipRTC as rt0_render
would, with the deferred path end (the default) and with the inline form, and
the define reaches the kernel (the two code objects differ, neither spills)."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def audit(tmp_path, tag, extra):
    env = dict(os.environ)
    env.pop("RT0_JIT_EXTRA", None)
    if extra:
        env["RT0_JIT_EXTRA"] = extra
    out = tmp_path / tag
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "jit_isa.py"), "c2", str(out)],
                       capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"rt0_jit_pass\s+vgpr (\d+) sgpr \d+ lds \S+ spill (\d+)", p.stdout)
    assert m, p.stdout
    n = re.search(r"rt0_jit_pass: (\d+) instructions", p.stdout)
    assert n, p.stdout
    return int(m.group(1)), int(m.group(2)), int(n.group(1))


def test_jit_isa_compiles_c2_with_and_without_deferred_path_end(tmp_path):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no ROCm LLVM tools")
    vgpr1, spill1, n1 = audit(tmp_path, "defer", None)
    vgpr0, spill0, n0 = audit(tmp_path, "inline", "-DRT0_PATH_END_DEFER=0")
    assert spill0 == 0 and spill1 == 0
    assert vgpr1 <= 64 and vgpr0 <= 64  # 8 waves per SIMD, as before (rt0_jit.cpp)
    assert n0 != n1  # the define selects another kernel
