"""The fold of workgroup slabs into table rows (query_amd/csrc/n1k_fold.h: one slab's words into a running accumulator, two
accumulators into one, accumulator -> row words) on the CPU: a stand-alone program (tests/host/fold_check.cpp, its own main, no
HIP) built with the host compiler under -fsanitize=address,undefined.  1, 2, 63, 64, 65 and 768 slabs x S = 2, 39, 1002 x every
aggregate kind x slots touched in random slabs, in exactly one, in none, and in all with int sums whose total passes 2^63, folded
in order and in fold_rows_kernel's geometry (64 and 128 slab-lanes), against a straightforward per-slot loop."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_slab_fold_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "fold_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "host", "fold_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "fold_check: ok" in out.stdout, out.stdout + out.stderr
