"""The batched vocoder stream push's C entry points on null arguments (no GPU): an error with a message, n_samples
cleared, never a crash."""
import ctypes as C
import os
import sys

import numpy as np

from q3t_testutil import REPO

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))


def _args(k):
    codes = [np.zeros((2, 16), np.int32) for _ in range(k)]
    pcm = [np.full(4096, 7.0, np.float32) for _ in range(k)]
    carr = (C.c_void_p * k)(*[c.ctypes.data for c in codes])
    parr = (C.c_void_p * k)(*[p.ctypes.data for p in pcm])
    nf = (C.c_int32 * k)(*[2] * k)
    cap = (C.c_int64 * k)(*[4096] * k)
    ns = (C.c_int64 * k)(*[-1] * k)
    return codes, pcm, carr, parr, nf, cap, ns


def test_null_arguments():
    import q3t
    lib = q3t.lib()
    err = lambda: lib.q3t_last_error().decode()
    # a null streams array
    codes, pcm, carr, parr, nf, cap, ns = _args(2)
    assert lib.q3t_vocoder_stream_push_batch(None, 2, carr, nf, parr, cap, ns) != 0
    assert "null argument" in err()
    assert list(ns) == [0, 0]
    # a null entry
    codes, pcm, carr, parr, nf, cap, ns = _args(2)
    harr = (C.c_void_p * 2)(None, None)
    assert lib.q3t_vocoder_stream_push_batch(harr, 2, carr, nf, parr, cap, ns) != 0
    assert "null vocoder stream" in err()
    assert list(ns) == [0, 0] and all((p == 7.0).all() for p in pcm)
    # no streams
    for k in (0, -3):
        codes, pcm, carr, parr, nf, cap, ns = _args(1)
        assert lib.q3t_vocoder_stream_push_batch(harr, k, carr, nf, parr, cap, ns) != 0
        assert "n_streams must be > 0" in err()
    # the other arrays
    assert lib.q3t_vocoder_stream_push_batch(harr, 2, None, nf, parr, cap, None) != 0
    assert "null argument" in err()


def test_last_groups_of_a_null_context():
    import q3t
    assert q3t.lib().q3t_vocoder_stream_last_groups(None) == -1
