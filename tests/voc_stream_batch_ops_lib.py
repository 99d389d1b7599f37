"""ctypes access to tests/voc_stream_batch_ops/libq3t_voc_stream_batch_ops.so, the test-only C entry points over the
batched vocoder-stream launchers (voc_kv_append_batch, voc_attn_cached_batch, voc_copy_batch)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


class Desc(C.Structure):
    """VocStreamDesc (csrc/vocoder_kernels.h) with device addresses as integers"""
    _fields_ = [("kc", C.c_uint64), ("vc", C.c_uint64), ("rope", C.c_uint64), ("layer_stride", C.c_int64),
                ("P", C.c_int32), ("n", C.c_int32), ("row0", C.c_int32), ("pad_", C.c_int32)]


def load():
    import hip_py   # loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launchers from it
    lib = C.CDLL(os.path.join(HERE, "voc_stream_batch_ops", "libq3t_voc_stream_batch_ops.so"))
    u64, i32 = C.c_uint64, C.c_int32
    tail = [C.c_char_p, C.c_int]
    lib.q3t_vsbo_kv_append_batch.argtypes = [u64, C.c_void_p, i32, i32, i32, i32] + tail
    lib.q3t_vsbo_attn_cached_batch.argtypes = [u64, u64, C.c_void_p, i32, i32, i32, i32] + tail
    lib.q3t_vsbo_copy_batch.argtypes = [C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int64), i32] + tail

    class Ops:
        DevBuf = hip_py.DevBuf

        @staticmethod
        def descs(items):
            """items: (kc, vc, rope, layer_stride, P, n, row0) per stream -> a ctypes array of Desc"""
            arr = (Desc * len(items))()
            for d, (kc, vc, rope, ls, P, n, row0) in zip(arr, items):
                d.kc, d.vc, d.rope, d.layer_stride, d.P, d.n, d.row0 = kc, vc, rope, ls, P, n, row0
            return arr

        @staticmethod
        def call(name, *args):
            err = C.create_string_buffer(512)
            rc = getattr(lib, "q3t_vsbo_" + name)(*args, err, 512)
            assert rc == 0, f"{name}: {err.value.decode()}"

        @staticmethod
        def copy_batch(copies):
            """copies: (src address, dst address, floats) per copy"""
            k = len(copies)
            src = (u64 * k)(*[c[0] for c in copies])
            dst = (u64 * k)(*[c[1] for c in copies])
            n = (C.c_int64 * k)(*[c[2] for c in copies])
            Ops.call("copy_batch", src, dst, n, k)
    return Ops
