"""k_pcm_out alone (csrc/pcm_out.hip) on raw f32 input, through the test-only shim tests/pcm_ops/: every rate, every
format, the lengths at which its indexing can go wrong, against the float64 restatement tests/pcm_out_ref.py.

Tolerance of the f32 output (derived in tests/test_pcm_out_ref.py, not measured): |d| <= gamma_K * sum_k |taps * x| per
sample against the float64 sum over the same f32 taps.  s16 and mu-law are compared exactly: s16 with the truncation
rule applied in numpy float32 to the kernel's own f32 output of the same case, mu-law with the reference encode of the
kernel's own s16.  Every launch also checks the poisoned bytes around every output (pcm_ops_lib.run)."""
import numpy as np
import pytest

import pcm_out_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 7, 159, 160, 161, 1365, 1920, 4001)
FORMATS = (R.F32, R.S16, R.MULAW)
CUTS = ([1] * 40, [3, 157, 1, 1760], [1365, 1920, 1920])


@pytest.fixture(scope="module")
def run():
    import pcm_ops_lib
    return pcm_ops_lib.load()


def Stream(*a, **k):
    import pcm_ops_lib
    return pcm_ops_lib.Stream(*a, **k)


def signal(kind, n, seed=0):
    if kind == "uniform":
        return np.random.default_rng(seed + n).uniform(-1, 1, n).astype(np.float32)
    if kind == "step":        # full scale: the filter's overshoot exceeds 1 and meets the clamp
        x = np.zeros(n, np.float32)
        x[n // 3:] = 1.0
        return x
    # plateaus at +-1.5 and +-1.0 exactly, long enough for the filter to settle on them
    vals = np.array([1.5, -1.5, 1.0, -1.0], np.float32)
    return vals[(np.arange(n) // 37) % 4]


def offsets(fmt, j):
    """byte offset of the output inside its region: every alignment the format allows, odd ones for u8"""
    return {R.F32: (0, 4, 8, 12), R.S16: (0, 2, 4, 6), R.MULAW: (0, 1, 2, 3)}[fmt][j % 4]


def check_f32(y, x, rate, final, where):
    K = R.geometry(rate)[2]
    ref, bound = R.resample(x, rate, final=final, with_bound=True)
    assert len(y) == len(ref), where
    if K == 0:
        assert y.tobytes() == np.asarray(x, np.float32).tobytes(), where   # the bypass: bit for bit
        return
    d = np.abs(y.astype(np.float64) - ref)
    tol = R.gamma(K) * bound
    assert np.all(d <= tol), (where, float(d.max()), int(np.argmax(d - tol)))


@pytest.mark.parametrize("rate", R.RATES)
def test_every_length_format_and_input(run, rate):
    cases = [(n, kind, final) for n in LENGTHS for kind in ("uniform", "step", "clamp") for final in (False, True)]
    streams, pieces, finals = [], [], []
    for ci, (n, kind, final) in enumerate(cases):
        for fmt in FORMATS:
            streams.append(Stream(rate, fmt, offsets(fmt, ci)))
            pieces.append(signal(kind, n))
            finals.append(final)
    outs = run(streams, pieces, finals)          # ONE launch of len(cases) * 3 streams
    worst = 0.0
    for ci, (n, kind, final) in enumerate(cases):
        f32, s16, mu = outs[3 * ci: 3 * ci + 3]
        where = (rate, n, kind, final)
        assert len(f32) == len(s16) == len(mu) == R.num_samples(n, rate, final), where
        check_f32(f32, pieces[3 * ci], rate, final, where)
        assert np.array_equal(s16, R.to_s16(f32)), where
        assert np.array_equal(mu, R.mulaw_encode(s16)), where
        if kind != "uniform" and len(s16):
            worst = max(worst, float(np.max(np.abs(f32))))
    if rate != R.NATIVE:
        assert worst > 1.0      # the clamp was met: some sample of the step or the plateaus went past full scale
    # the carried history is the last K - 1 samples of [zeros | x | tail]
    K, D = R.geometry(rate)[2], R.geometry(rate)[3]
    for st, x, f in zip(streams, pieces, finals):
        allx = np.concatenate([np.zeros(max(K - 1, 0), np.float32), x, np.zeros(D if f else 0, np.float32)])
        assert np.array_equal(st.hist[:max(K - 1, 0)], allx[len(allx) - max(K - 1, 0):]), (rate, len(x), f)
        assert np.all(st.hist[max(K - 1, 0):] == 0)


@pytest.mark.parametrize("cuts", CUTS, ids=["ones40", "3_157_1_1760", "1365_1920_1920"])
def test_pieces_give_the_bytes_of_the_whole(run, cuts):
    """every rate and format in one launch per piece, the history carried on the device side of the shim"""
    combos = [(rate, fmt) for rate in R.RATES for fmt in FORMATS]
    x = signal("uniform", sum(cuts), seed=len(cuts))
    whole = run([Stream(r, f) for r, f in combos], [x] * len(combos), [True] * len(combos))
    streams = [Stream(r, f, offsets(f, i)) for i, (r, f) in enumerate(combos)]
    parts = [[] for _ in combos]
    pos = 0
    for j, c in enumerate(cuts):
        last = j == len(cuts) - 1
        outs = run(streams, [x[pos:pos + c]] * len(combos), [last] * len(combos))
        pos += c
        for i, o in enumerate(outs):
            parts[i].append(o)
            assert streams[i].n0 == R.num_samples(pos, combos[i][0], last)
    for i, combo in enumerate(combos):
        got = np.concatenate(parts[i])
        assert got.dtype == whole[i].dtype and got.tobytes() == whole[i].tobytes(), combo
    # and the whole run is the reference's (f32 within the bound), so the pieces are right, not merely consistent
    for i, (rate, fmt) in enumerate(combos):
        if fmt == R.F32:
            check_f32(whole[i], x, rate, True, (rate, "whole"))


def test_eight_streams_in_one_launch_equal_eight_single_launches(run):
    """different rates, formats, positions (one past 2^33 input samples: the 64-bit index), piece lengths, alignments"""
    spec = [(8000, R.MULAW, 0, 480), (12000, R.S16, 161, 7), (16000, R.F32, 1365, 1920), (22050, R.S16, 3, 1365),
            (24000, R.MULAW, 40, 161), (32000, R.F32, 7, 0), (44100, R.MULAW, 2, 159), (48000, R.S16, 1920, 3)]
    rng = np.random.default_rng(8)
    streams, pieces = [], []
    for j, (rate, fmt, first, n) in enumerate(spec):
        st = Stream(rate, fmt, offsets(fmt, j + 1))
        if first:
            run([st], [rng.uniform(-1, 1, first).astype(np.float32)])     # brings it to its position and history
        streams.append(st)
        pieces.append(rng.uniform(-1, 1, n).astype(np.float32))
    far = streams[2]                    # (16000, F32): moved far out, with a history of its own
    K = R.geometry(far.rate)[2]
    far.hist[:K - 1] = rng.uniform(-1, 1, K - 1).astype(np.float32)
    far.s0 = 2 ** 33 + 10                # a multiple of M = 3: the first output reads the oldest carried sample
    far.n0 = R.num_samples(far.s0, far.rate)
    far_hist = far.hist.copy()
    finals = [j % 2 == 1 for j in range(8)]
    singles = [s.copy() for s in streams]
    together = run(streams, pieces, finals)
    for j in range(8):
        alone = run([singles[j]], [pieces[j]], [finals[j]])[0]
        assert together[j].tobytes() == alone.tobytes(), spec[j]
        assert np.array_equal(streams[j].hist, singles[j].hist), spec[j]
    # the far stream against the reference at the same position with the same history
    ref = R.RefStream(far.rate)
    ref.hist, ref.s0, ref.n0 = far_hist[:K - 1].astype(np.float64), 2 ** 33 + 10, R.num_samples(2 ** 33 + 10, far.rate)
    want = ref.push(pieces[2], final=finals[2])
    d = np.abs(together[2].astype(np.float64) - want)
    assert len(want) == len(together[2]) and np.all(d <= R.gamma(K) * ref.last_bound), float(d.max())
