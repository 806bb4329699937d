"""bench.py --dump-outputs on the host: the last step's groups as .npy files (values as numbers, tags beside them, groups
sorted by key unless the plan orders them, large results cut to a fixed sample under 64 MB), and --steps that cannot time
anything is refused."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from query_amd import _ffi  # noqa: E402
from query_amd.gpu_operator import GpuFilterGroup  # noqa: E402

VDT = GpuFilterGroup._VALUE_DT


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_groups_sorted_by_key_with_values_by_tag(tmp_path):
    ng = 50
    codes = np.random.default_rng(3).permutation(ng)
    keys = np.zeros((ng, 1), VDT)
    keys["tag"], keys["v"] = _ffi.T_STRING, codes[:, None]
    aggs = np.zeros((ng, 1), VDT)
    aggs["tag"], aggs["v"] = _ffi.T_INT, (codes * 10 - 7).astype(np.int64).view(np.uint64)[:, None]
    aggs["tag"][0, 0], aggs["v"][0, 0] = _ffi.T_FLOAT, np.array([2.5]).view(np.uint64)[0]
    aggs["tag"][1, 0], aggs["v"][1, 0] = _ffi.T_NULL, 12345
    bench.dump_outputs(str(tmp_path), {"keys": keys, "aggs": aggs}, bench.workloads()["config2"])
    d = _load(str(tmp_path))
    assert sorted(d) == ["agg_tags", "aggs", "key_tags", "keys"]
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert (d["keys"][:, 0] == np.arange(ng)).all() and (d["key_tags"] == _ffi.T_STRING).all()
    want = np.arange(ng) * 10.0 - 7.0
    want[codes[0]], want[codes[1]] = 2.5, 0.0
    assert (d["aggs"][:, 0] == want).all()
    assert d["agg_tags"][codes[0], 0] == _ffi.T_FLOAT and d["agg_tags"][codes[1], 0] == _ffi.T_NULL


def test_dump_of_a_large_result_is_a_fixed_sample_under_64_mb(tmp_path):
    ng = 6_400_000
    keys = np.zeros((ng, 2), VDT)
    keys["tag"], keys["v"] = _ffi.T_INT, np.arange(2 * ng, dtype=np.uint64).reshape(ng, 2)
    aggs = np.zeros((ng, 1), VDT)
    aggs["tag"] = _ffi.T_INT
    wl = bench.workloads()["config5_keys"]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"keys": keys, "aggs": aggs}, wl)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) < 64 << 20
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert (a["keys"][:, 0] == 2 * a["groups_index"]).all()


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
