"""The ownership rules of csrc/host_util.hpp (DevBuf, DevArr, reserve_group) without a GPU: tests/host_util_check.hip is a
stand-alone program that backs the header's three allocation hooks with malloc / free, a count of live allocations and a
"fail the k-th allocation" knob.  Its host side is built under AddressSanitizer + UBSan and it runs as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_buffer_ownership_rules_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_util_check")
    build = subprocess.run(
        [HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Werror", "-Wno-unused-function",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
         "-o", exe, os.path.join(ROOT, "tests", "host_util_check.hip")],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "host_util_check: ok" in run.stdout
