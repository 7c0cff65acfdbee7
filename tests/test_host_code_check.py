"""The device-free host code on its own (tools/hostcheck/host_code_check.cpp): the policy block packers of
pcg_policy_pack.hpp against the layout the kernel headers document, and the disk cache of pcg_jit_cache.hpp against every
file it must refuse.  Built here with the plain host compiler; tools/hostcheck/run.sh builds the same program under
sanitizers.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_check_passes(tmp_path):
    exe = str(tmp_path / "host_code_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tools", "hostcheck", "host_code_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert "465 shapes" in last, last
