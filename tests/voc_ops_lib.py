"""ctypes access to tests/ops/libq3t_ops.so, the test-only C entry points over the vocoder kernel launchers."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GENERIC, MT, PD = 1, 2, 3      # q3t::ConvKernel::family


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("x", "xh", "snake_a", "snake_ib", "w", "y", "y16", "y16_a", "y16_ib", "bias",
                                          "scale", "resid", "ct_w")] + \
               [("xbs", C.c_int64), ("ybs", C.c_int64)] + \
               [(n, C.c_int32) for n in ("T_in", "C_in", "C_out", "M", "n_taps", "dil", "pad", "so", "ob", "ldy", "act",
                                         "nb", "ct_k", "ct_st", "ct_trim", "T_out")]


class ResDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("xh", "x", "y", "y16", "w1", "w2", "b1", "a2", "ib2", "b2", "an", "ibn")] + \
               [("bs", C.c_int64), ("T", C.c_int32), ("dil", C.c_int32), ("nb", C.c_int32), ("pad_", C.c_int32)]


def load():
    """the shim's entry points (needs no GPU: conv_kernel is host arithmetic)"""
    import hip_py   # loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launchers from it
    lib = C.CDLL(os.path.join(HERE, "ops", "libq3t_ops.so"))
    u64, i32, i64, f32 = C.c_uint64, C.c_int32, C.c_int64, C.c_float
    tail = [C.c_char_p, C.c_int]
    lib.q3t_ops_conv.argtypes = [C.POINTER(ConvDesc)] + tail
    lib.q3t_ops_conv_kernel.argtypes = [C.POINTER(ConvDesc), C.POINTER(i32)]
    lib.q3t_ops_resunit96.argtypes = [C.POINTER(ResDesc)] + tail
    lib.q3t_ops_snake_f16.argtypes = [u64, u64, u64, u64, i64, i32] + tail
    lib.q3t_ops_norm_f16.argtypes = [u64, u64, u64, f32, i32, u64, i32, i32] + tail
    lib.q3t_ops_conv_out1.argtypes = [u64, u64, u64, u64, i32, i32, i32, i32] + tail
    lib.q3t_ops_dwconv.argtypes = [u64, u64, u64, u64, i32, i32, i32, i32] + tail
    lib.q3t_ops_attn_prefill.argtypes = [u64, u64, u64, i32, i32, i32, i32] + tail

    class Ops:
        DevBuf = hip_py.DevBuf

        @staticmethod
        def call(name, *args):
            err = C.create_string_buffer(512)
            rc = getattr(lib, "q3t_ops_" + name)(*args, err, 512)
            assert rc == 0, f"{name}: {err.value.decode()}"

        @staticmethod
        def kernel(d):
            out = (i32 * 6)()
            lib.q3t_ops_conv_kernel(C.byref(d), out)
            return tuple(out)
    return Ops
