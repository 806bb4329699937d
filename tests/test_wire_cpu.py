"""The arithmetic of the exchange's regions (query_amd/csrc/n1k_wire.h: capacity rounding, the layout of a packed row region,
where the regions of a collective lie in their buffers, usual buffers or scratch regions for a voided step) on the CPU: a
stand-alone program (tests/host/wire_check.cpp, its own main, no HIP) built with the host compiler under
-fsanitize=address,undefined.  World sizes 1, 2, 3 and 8 x DICT32 / TAGGED64 / mixed columns x capacities of one quantum, large
and with one hot owner x communicator buffers absent, sized by a smaller step, exact and sized by a larger step: every region
inside its extent, none overlapping, offsets on 16 and lengths on 128 bytes, the receiver's layout the sender's."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_region_arithmetic_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "wire_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "host", "wire_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "wire_check: ok" in out.stdout, out.stdout + out.stderr
