"""ctypes access to tests/voc_stream_ops/libq3t_voc_stream_ops.so, the test-only C entry points over the vocoder
stream's attention launchers (voc_kv_append, voc_attn_cached)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    import hip_py   # loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launchers from it
    lib = C.CDLL(os.path.join(HERE, "voc_stream_ops", "libq3t_voc_stream_ops.so"))
    u64, i32 = C.c_uint64, C.c_int32
    tail = [C.c_char_p, C.c_int]
    lib.q3t_vso_kv_append.argtypes = [u64, u64, u64, u64, i32, i32, i32, i32] + tail
    lib.q3t_vso_attn_cached.argtypes = [u64, u64, u64, u64, i32, i32, i32, i32] + tail

    class Ops:
        DevBuf = hip_py.DevBuf

        @staticmethod
        def call(name, *args):
            err = C.create_string_buffer(512)
            rc = getattr(lib, "q3t_vso_" + name)(*args, err, 512)
            assert rc == 0, f"{name}: {err.value.decode()}"
    return Ops
