"""CPU tests of the output stage's float64 restatement (tests/pcm_out_ref.py) and of the host-only helpers of the C ABI
(q3t_pcm_taps, q3t_pcm_num_samples, q3t_pcm_bytes_per_sample): the reference must meet the response figures on its
own, the library's table must be the reference's, and each wrong variant of the reference must move the output beyond
the tolerance tests/test_gpu_pcm_ops.py allows the kernel -- otherwise that comparison would not see the mistake.

The f32 tolerance (derived, not measured): against the float64 sum over the same f32 taps, a chain of K fmaf steps from
0.0f errs by at most gamma_K * sum_k |taps * x|, gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 3.1: each step rounds once)."""
import os
import sys

import numpy as np
import pytest

import pcm_out_ref as R
from q3t_testutil import REPO

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
RESAMPLED = [r for r in R.RATES if r != R.NATIVE]


def q3t_mod():
    import q3t
    return q3t


def gain_db(rate, freq):
    """gain of a unit sine of `freq` Hz, 1 s at 24 kHz, through the f32-rounded taps in float64: RMS over the middle
    half of the output against the sine's own RMS"""
    t = np.arange(R.NATIVE, dtype=np.float64) / R.NATIVE
    y = R.resample(np.sin(2 * np.pi * freq * t), rate, final=False)
    mid = y[len(y) // 4: len(y) - len(y) // 4]
    return 20 * np.log10(np.sqrt(np.mean(mid * mid)) / np.sqrt(0.5))


# ------------------------------------------------------------------------------------------------ the filter itself
@pytest.mark.parametrize("rate", RESAMPLED)
def test_reference_passband_is_flat(rate):
    nyq = min(rate, R.NATIVE) / 2.0
    for frac in (0.05, 0.5):
        g = gain_db(rate, frac * nyq)
        print(f"rate {rate}: gain at {frac} of Nyquist {g:+.5f} dB")
        assert abs(g) <= 0.01, (rate, frac, g)
    g = gain_db(rate, 0.8 * nyq)
    print(f"rate {rate}: gain at 0.8 of Nyquist {g:+.4f} dB")
    assert g >= -0.5, (rate, g)


@pytest.mark.parametrize("rate", [8000, 12000, 16000])
def test_reference_rejects_what_would_alias(rate):
    g = gain_db(rate, 1.15 * rate / 2.0)
    print(f"rate {rate}: tone at 1.15 x output Nyquist comes out at {g:.2f} dB")
    assert g <= -90.0, (rate, g)


def test_native_rate_is_the_identity():
    x = np.random.default_rng(0).uniform(-1, 1, 1000).astype(np.float32)
    x[3] = -0.0
    assert R.geometry(24000) == (1, 1, 0, 0)
    y = R.resample(x, 24000, dtype=np.float32)
    assert y.tobytes() == x.tobytes()
    assert R.num_samples(1000, 24000, True) == 1000


def test_geometry_table():
    """the figures the issue and DESIGN 2c state: the table is at most 160 x 35 floats, the history at most 96"""
    want = {8000: (1, 3, 97, 48), 12000: (1, 2, 65, 32), 16000: (2, 3, 49, 24), 22050: (147, 160, 35, 18),
            32000: (4, 3, 33, 16), 44100: (147, 80, 33, 16), 48000: (2, 1, 33, 16)}
    for rate, g in want.items():
        assert R.geometry(rate) == g, rate
        L, M, K, _ = g
        assert L * K <= 160 * 35 and K - 1 <= 96 and M <= 3 * L
    with pytest.raises(ValueError):
        R.geometry(11025)


# ------------------------------------------------------------------------------------------------ the library's helpers
@pytest.mark.parametrize("rate", R.RATES)
def test_library_taps_are_the_reference_design(rate):
    L, M, K, taps = q3t_mod().pcm_taps(rate)
    assert (L, M, K) == R.geometry(rate)[:3]
    ref = R.taps32(rate)
    assert taps.shape == ref.shape
    if K == 0:
        return
    # the two I0 evaluations may round a tap differently: at most 1 f32 ulp per tap (np.spacing of the larger one)
    ulp = np.spacing(np.maximum(np.abs(taps), np.abs(ref)).astype(np.float32))
    assert np.all(np.abs(taps.astype(np.float64) - ref.astype(np.float64)) <= ulp)
    assert np.count_nonzero(taps != ref) <= taps.size // 100   # and nearly all are the same float


def test_library_taps_errors_and_capacity():
    q3t, C = q3t_mod(), __import__("ctypes")
    lib = q3t.lib()
    L, M, K = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.q3t_pcm_taps(11025, C.byref(L), C.byref(M), C.byref(K), None, 0) != 0
    msg = lib.q3t_last_error().decode()
    assert "11025" in msg and all(str(r) in msg for r in R.RATES), msg
    buf = np.zeros(48, np.float32)
    assert lib.q3t_pcm_taps(16000, C.byref(L), C.byref(M), C.byref(K), buf.ctypes.data, 48) != 0   # needs 2 * 49
    assert "cap" in lib.q3t_last_error().decode()
    assert lib.q3t_pcm_taps(16000, None, None, None, None, 0) == 0


def test_library_num_samples_matches_the_formula():
    q3t = q3t_mod()
    for rate in R.RATES:
        L, M, K, D = R.geometry(rate)
        for final in (False, True):
            got = np.array([q3t.pcm_num_samples(S, rate, final) for S in range(4001)])
            S = np.arange(4001) + (D if final else 0)
            assert np.array_equal(got, -(-(S * L) // M)), (rate, final)
    assert q3t.pcm_num_samples(100, 11025) == -1
    assert q3t.pcm_num_samples(100, 0) == -1
    lib = q3t.lib()
    assert [lib.q3t_pcm_bytes_per_sample(f) for f in (0, 1, 2, 3, -1)] == [4, 2, 1, 0, 0]


# ------------------------------------------------------------------------------------------------ formats
def test_mulaw_known_answers_and_monotone():
    assert list(R.mulaw_encode(np.array([0, 32767, -32768], np.int16))) == [0xFF, 0x80, 0x00]
    # further G.711 anchors: the smallest negative value, the segment edges
    assert list(R.mulaw_encode(np.array([-1, 1, 3, 4], np.int16))) == [0x7F, 0xFF, 0xFF, 0xFE]
    allv = np.arange(-32768, 32768).astype(np.int16)
    dec = R.mulaw_decode(R.mulaw_encode(allv))
    assert np.all(np.diff(dec) >= 0), "the encode is not monotone over the s16 range"
    assert len(np.unique(R.mulaw_encode(allv))) == 256   # every code is used: 0x7F by -1 .. -3, 0xFF by 0 .. 3
    # the expansion stays within one step of the value's segment (8 << exponent) below the clip
    step = 8 << ((~R.mulaw_encode(allv).astype(np.int32) >> 4) & 7)
    inside = np.abs(allv.astype(np.int32)) <= 32635
    assert np.all(np.abs(dec - allv.astype(np.int32))[inside] <= step[inside])


def test_s16_truncates_toward_zero_and_clamps():
    y = np.array([0.0, 1.0, -1.0, 1.5, -1.5, 0.5, -0.5, 0.99999, 1e-5], np.float32)
    assert list(R.to_s16(y)) == [0, 32767, -32767, 32767, -32767, 16383, -16383, 32766, 0]


# ------------------------------------------------------------------------------------------------ chunk invariance
CUTS = ([1] * 40, [3, 157, 1, 1760], [1365, 1920, 1920], [0, 5, 0, 200, 1])


@pytest.mark.parametrize("rate", R.RATES)
def test_reference_is_chunk_invariant(rate):
    rng = np.random.default_rng(rate)
    for cuts in CUTS:
        x = rng.uniform(-1, 1, sum(cuts)).astype(np.float32)
        whole = R.resample(x, rate, final=True)
        st = R.RefStream(rate)
        parts, pos = [], 0
        for j, c in enumerate(cuts):
            parts.append(st.push(x[pos:pos + c], final=j == len(cuts) - 1))
            pos += c
            assert st.n0 == R.num_samples(pos, rate, j == len(cuts) - 1)
        got = np.concatenate(parts)
        assert got.dtype == whole.dtype and got.tobytes() == whole.tobytes(), (rate, cuts)


def test_reference_float32_run_stays_inside_the_bound():
    """the kernel's own loop restated in float32 numpy: inside gamma_K * sum |taps * x| of the float64 sum"""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, 4001).astype(np.float32)
    for rate in RESAMPLED:
        K = R.geometry(rate)[2]
        y64, bound = R.resample(x, rate, with_bound=True)
        y32 = R.resample(x, rate, dtype=np.float32)
        d = np.abs(y32.astype(np.float64) - y64)
        assert np.all(d <= R.gamma(K) * bound), rate
        print(f"rate {rate}: float32 loop max |d| {d.max():.3g}, bound {float((R.gamma(K) * bound).max()):.3g}")


# ------------------------------------------------------------------------------------------------ mutations
def beyond_tolerance(y_wrong, y_ref, bound, K):
    n = min(len(y_wrong), len(y_ref))
    return np.count_nonzero(np.abs(y_wrong[:n] - y_ref[:n]) > R.gamma(K) * bound[:n])


@pytest.mark.parametrize("rate", RESAMPLED)
def test_mutations_move_the_output_beyond_the_tolerance(rate):
    rng = np.random.default_rng(rate + 1)
    x = rng.uniform(-1, 1, 1921).astype(np.float32)
    L, M, K, D = R.geometry(rate)
    ref, bound = R.resample(x, rate, with_bound=True)
    # one tap dropped (the centre one, the last one, the first one)
    for k in (K // 2, K - 1, 0):
        assert beyond_tolerance(R.resample(x, rate, drop_tap=k), ref, bound, K) > 0, ("tap", k)
    # phase off by one: t = n * M + 1
    assert beyond_tolerance(R.resample(x, rate, phase_off=1), ref, bound, K) > len(ref) // 2
    # history one sample short.  The oldest carried sample x[s0 - (K - 1)] is read only by an output whose newest input
    # is x[s0] itself, which exists when the cut s0 is a multiple of M (then n0 * M = s0 * L, phase 0), and it meets the
    # filter's outermost tap, about 1e-5: cut at multiples of M and make that sample the loud one of a quiet signal
    c1, c2 = M * (700 // M), M * (1300 // M)
    x = (x * np.float32(1e-3)).astype(np.float32)
    x[c1 - (K - 1)] = x[c2 - (K - 1)] = 1.0
    ref, bound = R.resample(x, rate, with_bound=True)
    st = R.RefStream(rate, hist_short=1)
    got = np.concatenate([st.push(x[:c1]), st.push(x[c1:c2]), st.push(x[c2:], final=True)])
    assert len(got) == len(ref) and beyond_tolerance(got, ref, bound, K) > 0
    # and the unmutated chunked run is the whole run, so the difference is the mutation's doing
    st = R.RefStream(rate)
    got = np.concatenate([st.push(x[:c1]), st.push(x[c1:c2]), st.push(x[c2:], final=True)])
    assert beyond_tolerance(got, ref, bound, K) == 0


def test_rounding_where_truncation_is_specified_changes_the_s16():
    y = np.random.default_rng(9).uniform(-1, 1, 4096).astype(np.float32)
    a, b = R.to_s16(y), R.to_s16(y, rounding=True)
    assert np.count_nonzero(a != b) > len(y) // 4          # the s16 comparison is exact: any difference fails it
    assert np.max(np.abs(a.astype(np.int32) - b.astype(np.int32))) == 1
