"""ctypes access to tests/pcm_ops/libq3t_pcm_ops.so, the test-only C entry point over the output stage's launchers
(pcm_out, pcm_out_hist): k_pcm_out alone on raw f32 input, any number of streams in one launch."""
import ctypes as C
import os

import numpy as np

import pcm_out_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_HIST = 96      # kPcmMaxHist (csrc/pcm_out.h)
GUARD = 64         # poisoned bytes on each side of an output
POISON = 0xA5


class Stream:
    """one stream's share of a launch: its state travels with it from launch to launch"""

    def __init__(self, rate, fmt, out_off=0):
        self.rate, self.fmt, self.out_off = rate, fmt, out_off    # out_off: extra bytes before the output (alignment)
        self.hist = np.zeros(MAX_HIST, np.float32)
        self.s0 = 0
        self.n0 = 0

    def copy(self):
        c = Stream(self.rate, self.fmt, self.out_off)
        c.hist, c.s0, c.n0 = self.hist.copy(), self.s0, self.n0
        return c


def load():
    import hip_py   # noqa: F401  loads libq3t.so (and its HIP runtime) first: the shim resolves the q3t:: launchers from it
    lib = C.CDLL(os.path.join(HERE, "pcm_ops", "libq3t_pcm_ops.so"))
    P = C.c_void_p
    lib.q3t_pcmo_run.argtypes = [C.c_int32, P, P, P, P, P, P, P, P, P, P, P, C.c_char_p, C.c_int]

    def run(streams, pieces, finals=None):
        """ONE launch: stream j consumes pieces[j] (float32).  Returns each stream's output in its format; checks the
        count against the formula and that every byte of the poisoned region around the output is untouched"""
        n = len(streams)
        finals = [False] * n if finals is None else list(finals)
        xs = [np.ascontiguousarray(p, np.float32) for p in pieces]
        bps = [np.dtype(R.DTYPES[st.fmt]).itemsize for st in streams]
        want = [R.num_samples(st.s0 + len(x), st.rate, f) - st.n0 for st, x, f in zip(streams, xs, finals)]
        regions = [np.full(GUARD + st.out_off + w * b + GUARD, POISON, np.uint8) for st, w, b in zip(streams, want, bps)]

        def arr(ct, vals):
            return (ct * n)(*vals)
        xp = arr(C.c_void_p, [x.ctypes.data for x in xs])
        hp = arr(C.c_void_p, [st.hist.ctypes.data for st in streams])
        rp = arr(C.c_void_p, [r.ctypes.data for r in regions])
        n_out = (C.c_int64 * n)()
        err = C.create_string_buffer(512)
        rc = lib.q3t_pcmo_run(n, xp, arr(C.c_int32, [len(x) for x in xs]), hp, arr(C.c_int32, [st.rate for st in streams]),
                              arr(C.c_int32, [st.fmt for st in streams]), arr(C.c_int64, [st.s0 for st in streams]),
                              arr(C.c_int32, [1 if f else 0 for f in finals]), rp,
                              arr(C.c_int64, [len(r) for r in regions]),
                              arr(C.c_int64, [GUARD + st.out_off for st in streams]), n_out, err, 512)
        assert rc == 0, err.value.decode()
        outs = []
        for j, (st, r, w, b) in enumerate(zip(streams, regions, want, bps)):
            assert n_out[j] == w, (j, n_out[j], w)
            lo = GUARD + st.out_off
            assert np.all(r[:lo] == POISON), f"stream {j}: bytes before the output were written"
            assert np.all(r[lo + w * b:] == POISON), f"stream {j}: bytes after the output were written"
            outs.append(r[lo:lo + w * b].copy().view(R.DTYPES[st.fmt]) if w else np.zeros(0, R.DTYPES[st.fmt]))
            st.s0 += len(xs[j])
            st.n0 += w
        return outs
    return run
