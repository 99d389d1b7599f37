"""Queue deliveries, host side (no GPU): the new C entry points are exported with the documented signatures and fail
with a message on null arguments, and Engine.generate_queue_stream validates its arguments before it touches a
device."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from q3t_testutil import REPO

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))


def _header():
    with open(os.path.join(REPO, "include", "q3t_backend.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def test_symbols_and_documented_signatures():
    import q3t
    lib = q3t.lib()
    for name in ("q3t_generate_queue_stream", "q3t_vocoder_stream_reset"):
        assert hasattr(lib, name), name
    h = _header()
    assert ("typedef int (*q3t_queue_cb)(void *user, int32_t n, const int32_t *utt, const int32_t *const *codes, "
            "const int32_t *n_frames, const int32_t *final, int32_t *stop);") in h
    assert ("int q3t_generate_queue_stream(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens, "
            "const float *const *speaker, const q3t_gen_params *p, int32_t *codes , int32_t *n_frames, int32_t max_active, "
            "q3t_queue_cb cb, void *user, int32_t interval);") in h
    assert "int q3t_vocoder_stream_reset(q3t_voc_stream *s);" in h
    # the ctypes mirror: 12 arguments, the callback with 7
    assert len(lib.q3t_generate_queue_stream.argtypes) == 12
    assert len(q3t.QUEUE_CB._argtypes_) == 7 and q3t.QUEUE_CB._restype_ is C.c_int


def test_null_arguments():
    import q3t
    lib = q3t.lib()
    err = lambda: lib.q3t_last_error().decode()
    nf = np.zeros(1, np.int32)
    cb = q3t.QUEUE_CB(lambda *a: 1)
    assert lib.q3t_generate_queue_stream(None, 0, None, nf, None, None, None, nf, 0, cb, None, 12) != 0
    assert err().strip()
    assert lib.q3t_vocoder_stream_reset(None) != 0
    assert "null vocoder stream" in err()


def test_python_wrapper_validates_before_touching_a_device():
    import q3t
    sig = inspect.signature(q3t.Engine.generate_queue_stream)
    assert list(sig.parameters)[:7] == ["self", "prompts", "on_batch", "interval", "speakers", "max_active", "want_codes"]
    assert sig.parameters["interval"].default == 12 and sig.parameters["want_codes"].default is True
    assert callable(q3t.VocoderStream.reset)
    eng = q3t.Engine.__new__(q3t.Engine)   # no context behind it: a call that got past the checks would fail differently
    eng.h = None
    with pytest.raises(TypeError):
        eng.generate_queue_stream([[1, 2, 3]], None)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            eng.generate_queue_stream([[1, 2, 3]], lambda e: None, interval=bad)
    with pytest.raises(ValueError):
        eng.generate_queue_stream([[1, 2, 3]], lambda e: None, speakers=[])
