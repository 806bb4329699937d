"""DevBuf / PinBuf (query_amd/csrc/n1k_buf.h), the owners of the engine's device and pinned memory, on the CPU: a stand-alone
program (tests/host/devbuf_check.cpp, its own main, the four HIP allocation calls stubbed by malloc / free and a ledger) built
with the host compiler under -fsanitize=address,undefined.  Move construction, move assignment onto a full buffer, self-move,
ensure's growth, release then reuse, a failed allocation, a vector of them resized, and the byte count back at zero."""
import os
import subprocess

from query_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owners_under_the_host_sanitizers(tmp_path):
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))  # <rocm>/bin/hipcc: the HIP headers' types only
    exe = str(tmp_path / "devbuf_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-o", exe,
                           os.path.join(HERE, "host", "devbuf_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "devbuf_check: ok" in out.stdout, out.stdout + out.stderr
