"""ctypes access to tests/attn_ops/libq3t_attn_ops.so, the test-only C entry points over the decode / prefill attention
launchers (the counterpart of voc_ops_lib for tests/test_gpu_attn_ops.py)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


class AttnDesc(C.Structure):
    """Q3tOpsAttn: q3t::AttnParams field by field (dbg stays null)"""
    _fields_ = [(n, C.c_uint64) for n in ("qkv", "qn", "kn", "rope", "pos", "kc", "vc", "part", "ticket", "out", "qkv_tab",
                                          "tab_tok", "tab_row0")] + \
               [("eps", C.c_float)] + \
               [(n, C.c_int32) for n in ("n_ctx", "S", "nH", "nKV", "D", "chunk", "seqk", "small", "max_splits", "tab_ld",
                                         "tab_col")]


class PrefillAttnDesc(C.Structure):
    """Q3tOpsPrefillAttn: q3t::PrefillAttnParams field by field"""
    _fields_ = [(n, C.c_uint64) for n in ("qkv", "qn", "kn", "rope", "kc", "vc", "slot", "out")] + \
               [("eps", C.c_float)] + \
               [(n, C.c_int32) for n in ("n_ctx", "n_utt", "plen", "nH", "nKV", "D", "pad_")]


def load():
    """the shim's entry points"""
    import hip_py   # loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launchers from it
    lib = C.CDLL(os.path.join(HERE, "attn_ops", "libq3t_attn_ops.so"))
    tail = [C.c_char_p, C.c_int]
    lib.q3t_ops_attn_decode.argtypes = [C.POINTER(AttnDesc)] + tail
    lib.q3t_ops_prefill_attn.argtypes = [C.POINTER(PrefillAttnDesc)] + tail

    class Ops:
        DevBuf = hip_py.DevBuf

        @staticmethod
        def call_rc(name, *args):
            """(rc, error text): the launchers' refusals return -1 and their message"""
            err = C.create_string_buffer(512)
            rc = getattr(lib, "q3t_ops_" + name)(*args, err, 512)
            return rc, err.value.decode()

        @staticmethod
        def call(name, *args):
            rc, msg = Ops.call_rc(name, *args)
            assert rc == 0, f"{name}: {msg}"
    return Ops
