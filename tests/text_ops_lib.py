"""ctypes access to tests/text_ops/libq3t_text_ops.so, the test-only C entry points over the text-feed launchers
(text_append, slot_hold, slot_release)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    import hip_py   # loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launchers from it
    lib = C.CDLL(os.path.join(HERE, "text_ops", "libq3t_text_ops.so"))
    u64, i32 = C.c_uint64, C.c_int32
    lib.q3t_to_append.argtypes = [u64] * 7 + [i32] * 6 + [C.c_char_p, C.c_int]
    lib.q3t_to_hold.argtypes = [u64] * 6 + [i32] * 3 + [C.c_char_p, C.c_int]

    class Ops:
        DevBuf = hip_py.DevBuf

        @staticmethod
        def call(name, *args):
            err = C.create_string_buffer(512)
            rc = getattr(lib, "q3t_to_" + name)(*args, err, 512)
            assert rc == 0, f"{name}: {err.value.decode()}"
    return Ops
