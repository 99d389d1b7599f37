"""The wave reduction helpers of the one-slot role kernels' bodies (csrc/q3t_common.h), one launch through
tests/reduce_ops/libq3t_reduce_ops.so, the op-level entry for them (as tests/attn_ops/ is for the attention launchers):

  group_sum<16>           DPP row steps, four neighbouring accumulators as in the role bodies, compiled as the role
                          kernels are (no SLP vectoriser: the steps fold into v_add_f32_dpp)
  wave_sum_d              DPP steps that leave their destination uninitialised (Q3T_DPP_BOUND=1), then the row swaps
  the QKV publish         group16_sum_scatter4 + rows_gather16 + scatter4_index (Q3T_QKV_SCATTER=1): 5 adds, two row swaps

(the last two are build knobs that are off in the library, having shown no gain; the library's own forms are the
references here)
each against the form it replaced or must equal, computed in the same launch over generic shuffles (ds_bpermute) and
zero-initialised DPP moves, and against the same trees in numpy.  Every step of every form adds the same two operands,
and IEEE addition is commutative, so every bit must be equal: 64 random vectors, and vectors of signed zeros, denormals
and 1e30 mixed with 1e-30.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _vectors():
    """f32 [nv][4][64] and f64 [nv][64]"""
    rng = np.random.default_rng(1234)
    f = [rng.standard_normal((64, 4, 64)).astype(np.float32)]
    d = [rng.standard_normal((64, 64))]
    # wide exponent range: partial sums of very different magnitude, cancellation
    f.append((rng.standard_normal((8, 4, 64)) * 10.0 ** rng.integers(-30, 31, (8, 4, 64))).astype(np.float32))
    d.append(rng.standard_normal((8, 64)) * 10.0 ** rng.integers(-200, 201, (8, 64)))
    # signed zeros: -0 + -0 = -0, -0 + +0 = +0
    z = np.where(rng.integers(0, 2, (4, 4, 64)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    z[0] = np.float32(-0.0)
    f.append(z)
    zd = np.where(rng.integers(0, 2, (4, 64)) == 1, -0.0, 0.0)
    zd[0] = -0.0
    d.append(zd)
    # denormals (f32 below 1.18e-38, f64 below 2.2e-308), alone and beside normal values
    den = (rng.integers(1, 1 << 22, (4, 4, 64)).astype(np.uint32) | (rng.integers(0, 2, (4, 4, 64)).astype(np.uint32) << 31))
    den = den.view(np.float32).copy()
    den[2:, :, ::5] = rng.standard_normal((2, 4, 13)).astype(np.float32) * np.float32(1e-37)
    f.append(den)
    dd = (rng.integers(1, 1 << 50, (4, 64)).astype(np.uint64) | (rng.integers(0, 2, (4, 64)).astype(np.uint64) << 63))
    dd = dd.view(np.float64).copy()
    dd[2:, ::5] = rng.standard_normal((2, 13)) * 1e-307
    d.append(dd)
    # 1e30 mixed with 1e-30, both signs
    m = np.where(rng.integers(0, 2, (4, 4, 64)) == 1, 1e30, 1e-30) * np.where(rng.integers(0, 2, (4, 4, 64)) == 1, -1.0, 1.0)
    f.append(m.astype(np.float32))
    md = np.where(rng.integers(0, 2, (4, 64)) == 1, 1e30, 1e-30) * np.where(rng.integers(0, 2, (4, 64)) == 1, -1.0, 1.0)
    d.append(md)
    return np.ascontiguousarray(np.concatenate(f)), np.ascontiguousarray(np.concatenate(d))


def _tree16(x):
    """group_sum<16> over the last axis (64 lanes) in numpy: the value of every lane after lane ^ 1, lane ^ 2,
    row_half_mirror and row_mirror steps, in the array's own precision"""
    l = np.arange(64)
    for src in (l ^ 1, l ^ 2, (l & ~7) | (7 - (l & 7)), (l & ~15) | (15 - (l & 15))):
        x = x + x[..., src]
    return x


@pytest.fixture(scope="module")
def forms():
    import hip_py
    lib = C.CDLL(os.path.join(HERE, "reduce_ops", "libq3t_reduce_ops.so"))
    lib.q3t_ops_reduce_forms.argtypes = [C.c_uint64] * 2 + [C.c_int] + [C.c_uint64] * 6 + [C.c_char_p, C.c_int]
    f, d = _vectors()
    nv = f.shape[0]
    assert d.shape == (nv, 64)
    bf, bd = hip_py.DevBuf(f), hip_py.DevBuf(d)
    outs = {"gs_new": (np.uint32, nv * 4 * 64), "gs_ref": (np.uint32, nv * 4 * 64), "ws_new": (np.uint64, nv * 64),
            "ws_ref": (np.uint64, nv * 64), "pub_new": (np.uint32, nv * 16), "pub_ref": (np.uint32, nv * 16)}
    bufs = {k: hip_py.DevBuf(np.full(n, 0x7fc00123, dt)) for k, (dt, n) in outs.items()}   # poisoned: every word is written
    err = C.create_string_buffer(512)
    rc = lib.q3t_ops_reduce_forms(bf.p, bd.p, nv, *[bufs[k].p for k in outs], err, 512)
    assert rc == 0, err.value.decode()
    got = {k: bufs[k].get(dt, n) for k, (dt, n) in outs.items()}
    for b in [bf, bd] + list(bufs.values()):
        b.close()
    return f, d, got


def test_group_sum16_bits(forms):
    f, _, got = forms
    new = got["gs_new"].reshape(f.shape)
    assert np.array_equal(new, got["gs_ref"].reshape(f.shape))
    with np.errstate(all="ignore"):
        assert np.array_equal(new, _tree16(f).view(np.uint32))


def test_wave_sum_d_bits(forms):
    _, d, got = forms
    new = got["ws_new"].reshape(d.shape)
    assert np.array_equal(new, got["ws_ref"].reshape(d.shape))
    l = np.arange(64)
    with np.errstate(all="ignore"):
        x = _tree16(d)
        x = x + x[..., l ^ 16]
        x = x + x[..., l ^ 32]
    assert np.array_equal(new, x.view(np.uint64))


def test_publish_reduce_scatter_bits(forms):
    f, _, got = forms
    nv = f.shape[0]
    new = got["pub_new"].reshape(nv, 16)
    assert np.array_equal(new, got["pub_ref"].reshape(nv, 16))
    with np.errstate(all="ignore"):
        s = _tree16(f).view(np.uint32)   # [nv][j][lane]: row 4j + g is accumulator j over lanes 16g .. 16g + 15
    want = s[:, :, ::16].reshape(nv, 16)
    assert np.array_equal(new, want)
