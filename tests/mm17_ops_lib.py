"""ctypes access to tests/mm17_ops/libq3t_mm17_ops.so, the test-only C entry points over resid_norm,
select_embed_norm and gemv (the launchers the 1.7B matrix-core path added shapes to)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    import hip_py   # loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launchers from it
    lib = C.CDLL(os.path.join(HERE, "mm17_ops", "libq3t_mm17_ops.so"))
    u64, i32, f32 = C.c_uint64, C.c_int32, C.c_float
    tail = [C.c_char_p, C.c_int]
    lib.q3t_m17_resid_norm.argtypes = [u64, u64, u64, i32, u64, f32, u64, u64, i32, i32] + tail
    lib.q3t_m17_select_embed_norm.argtypes = [u64, i32, i32, f32, u64, u64, i32, u64, u64, u64, i32, i32,
                                              u64, u64, u64, u64, i32, u64, u64, u64, u64, u64, u64, f32, i32, i32] + tail
    lib.q3t_m17_gemv.argtypes = [u64, i32, i32, i32, u64, i32, u64, u64, i32, u64, i32] + tail

    class Ops:
        DevBuf = hip_py.DevBuf

        @staticmethod
        def raw(name, *args):
            """(the entry's return value, its error text)"""
            err = C.create_string_buffer(512)
            rc = getattr(lib, "q3t_m17_" + name)(*args, err, 512)
            return rc, err.value.decode()

        @staticmethod
        def call(name, *args):
            """the entry's value (>= 0); an error of the launcher fails the test with its text"""
            rc, err = Ops.raw(name, *args)
            assert rc >= 0, f"{name}: {err}"
            return rc
    return Ops
