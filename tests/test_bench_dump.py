"""CPU: bench.py's --dump-outputs writer (dump_outputs).

Small outputs are written whole as float32; outputs above the byte limit are cut to a fixed sample (seed 0, ascending
flat indices) so that the files of two runs hold the same elements and stay within the limit together.
"""
import os
import sys

import numpy as np

from q3t_testutil import REPO

sys.path.insert(0, REPO)


def test_small_outputs_written_whole_as_float32(tmp_path):
    import bench
    codes = np.arange(2 * 8 * 16, dtype=np.int32).reshape(2, 8, 16) % 3072
    pcm = np.linspace(-1, 1, 2 * 100, dtype=np.float32).reshape(2, 100)
    d = str(tmp_path / "out" / "nested")
    bench.dump_outputs(d, {"codes": codes, "pcm": pcm})
    assert sorted(os.listdir(d)) == ["codes.npy", "pcm.npy"]
    c, p = np.load(os.path.join(d, "codes.npy")), np.load(os.path.join(d, "pcm.npy"))
    assert c.dtype == np.float32 and c.shape == codes.shape and np.array_equal(c, codes)
    assert p.dtype == np.float32 and p.shape == pcm.shape and np.array_equal(p, pcm)


def test_large_output_cut_to_a_fixed_sample_within_the_limit(tmp_path):
    import bench
    limit = 4000
    small = np.arange(100, dtype=np.int32)                   # 400 B: below its 2000 B share, kept whole
    big = np.random.default_rng(5).standard_normal((50, 100))  # 20 kB as float32: cut to 500 elements
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), {"small": small, "big": big}, limit=limit)
    a = {n: np.load(str(tmp_path / "a" / f"{n}.npy")) for n in ("small", "big")}
    b = {n: np.load(str(tmp_path / "b" / f"{n}.npy")) for n in ("small", "big")}
    assert np.array_equal(a["small"], small)
    assert a["big"].dtype == np.float32 and a["big"].shape == (500,)
    assert sum(v.nbytes for v in a.values()) <= limit
    assert np.array_equal(a["big"], b["big"])
    # the sample is elements of the flattened array at ascending indices drawn with seed 0
    idx = np.sort(np.random.default_rng(0).choice(big.size, 500, replace=False))
    assert np.array_equal(a["big"], big.astype(np.float32).ravel()[idx])
    assert bench.DUMP_LIMIT_BYTES <= 64 * 1000 * 1000
