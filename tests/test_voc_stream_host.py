"""The vocoder stream's C entry points on null handles (no GPU): an error with a message, never a crash."""
import ctypes as C
import os
import sys

import numpy as np

from q3t_testutil import REPO

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))


def test_null_handles():
    import q3t
    lib = q3t.lib()
    h = C.c_void_p(1234)
    assert lib.q3t_vocoder_stream_open(None, 64, C.byref(h)) != 0
    assert "null context" in lib.q3t_last_error().decode()
    assert not h.value, "*out must be cleared on failure"
    codes = np.zeros((2, 16), np.int32)
    pcm = np.zeros(4096, np.float32)
    ns = C.c_int64(-1)
    rc = lib.q3t_vocoder_stream_push(None, codes.ctypes.data_as(C.c_void_p), 2, pcm.ctypes.data_as(C.c_void_p), pcm.size,
                                     C.byref(ns))
    assert rc != 0 and ns.value == 0
    assert "null vocoder stream" in lib.q3t_last_error().decode()
    assert lib.q3t_vocoder_stream_samples(None) == -1
    assert lib.q3t_vocoder_stream_frames(None) == -1
    assert lib.q3t_vocoder_stream_halo(None) == -1
    lib.q3t_vocoder_stream_close(None)   # a no-op
