"""ctypes access to tests/queue_ops/libq3t_queue_ops.so, the test-only C entry point over the continuous-batching
queue's collection launcher (queue_collect)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    import hip_py   # loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launcher from it
    lib = C.CDLL(os.path.join(HERE, "queue_ops", "libq3t_queue_ops.so"))
    u64, i32 = C.c_uint64, C.c_int32
    lib.q3t_qo_collect.argtypes = [u64] * 8 + [i32] * 4 + [C.c_char_p, C.c_int]

    class Ops:
        DevBuf = hip_py.DevBuf

        @staticmethod
        def call(name, *args):
            err = C.create_string_buffer(512)
            rc = getattr(lib, "q3t_qo_" + name)(*args, err, 512)
            assert rc == 0, f"{name}: {err.value.decode()}"
    return Ops
