"""The output stage through the public API (q3t_vocoder_decode_out, q3t_vocoder_stream_set_output / _push_out /
_push_batch_out; Engine.vocoder(out=), VocoderStream.push(final=), Engine.vocoder_stream_push_batch(final=)) on the
`tiny` and `full` synthetic vocoders: the native rate is the plain decode bit for bit, pushes in any pattern give the
bytes of the one-shot call, a batched push gives the bytes of single pushes with one conversion launch, and every
error leaves the stream where it was.  Utterances of at most 40 frames; one decode per configuration is shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import pcm_out_ref as R
from q3t_testutil import REPO, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu

F_ALL = 40
SPECS = [(8000, R.S16), (22050, R.F32), (48000, R.MULAW)]
PATTERNS = [[1] * 16, [31, 8, 1], [7, 25, 1, 7]]


@pytest.fixture(scope="module", params=["tiny", "full"])
def setup(request):
    import q3t
    tts, tok = synth_dir(request.param)
    eng = q3t.Engine(None, tok, device=0)
    codes = [np.random.default_rng(700 + j).integers(0, 2048, size=(F_ALL, 16), dtype=np.int32) for j in range(5)]
    pcm = [eng.vocoder(c, 0) for c in codes]          # the decoder is causal: a prefix's decode is a prefix of this
    for a in codes + pcm:
        a.setflags(write=False)
    yield q3t, eng, codes, pcm
    eng.close()


def expect_error(q3t, fn, *needles):
    with pytest.raises(q3t.Q3TError) as e:
        fn()
    for n in needles:
        assert n in str(e.value), (n, str(e.value))


# ------------------------------------------------------------------------------------------------ one-shot
def test_native_rate_is_the_plain_decode(setup):
    q3t, eng, codes, pcm = setup
    f32 = eng.vocoder(codes[0], 0, out=(24000, q3t.PCM_F32))
    assert f32.dtype == np.float32 and f32.tobytes() == pcm[0].tobytes()
    s16 = eng.vocoder(codes[0], 0, out=q3t.PcmSpec(24000, q3t.PCM_S16))
    want = (np.clip(pcm[0], -1, 1) * np.float32(32767)).astype(np.int16)      # the WAV writer's bytes
    assert s16.dtype == np.int16 and s16.tobytes() == want.tobytes()
    mu = eng.vocoder(codes[0], 0, out=(24000, q3t.PCM_MULAW))
    assert mu.dtype == np.uint8 and np.array_equal(mu, R.mulaw_encode(want))
    chunked = eng.vocoder(codes[0], q3t.VOCODER_CHUNK40, out=(24000, q3t.PCM_F32))
    assert chunked.tobytes() == eng.vocoder(codes[0], q3t.VOCODER_CHUNK40).tobytes()


@pytest.mark.parametrize("rate,mode", [(22050, 0), (8000, 0), (48000, 0), (16000, 1)])
def test_one_shot_is_the_reference_filter_of_the_plain_decode(setup, rate, mode):
    """f32 within the fma chain's bound of the float64 run over the same f32 taps; s16 and mu-law by their exact rules
    from the call's own f32 / s16 (the conversion is per sample, so the three calls see the same filtered values)"""
    q3t, eng, codes, pcm = setup
    x = pcm[1] if mode == 0 else eng.vocoder(codes[1], mode)
    y = eng.vocoder(codes[1], mode, out=(rate, q3t.PCM_F32))
    ref, bound = R.resample(x, rate, final=True, with_bound=True)
    assert len(y) == len(ref) == q3t.pcm_num_samples(len(x), rate, True)
    d = np.abs(y.astype(np.float64) - ref)
    assert np.all(d <= R.gamma(R.geometry(rate)[2]) * bound), float(d.max())
    s16 = eng.vocoder(codes[1], mode, out=(rate, q3t.PCM_S16))
    assert np.array_equal(s16, R.to_s16(y))
    assert np.array_equal(eng.vocoder(codes[1], mode, out=(rate, q3t.PCM_MULAW)), R.mulaw_encode(s16))


# ------------------------------------------------------------------------------------------------ streams
@pytest.mark.parametrize("spec", SPECS, ids=["8000_s16", "22050_f32", "48000_mulaw"])
def test_pushes_give_the_bytes_of_the_one_shot_call(setup, spec):
    q3t, eng, codes, pcm = setup
    rate, fmt = spec
    with eng.vocoder_stream(max_frames=F_ALL, out=spec) as st:
        for pi, pat in enumerate(PATTERNS):
            if pi:
                st.reset()                                  # the spec stays, the stage starts over
                assert st.frames == 0 and st.out_samples == 0
            F = sum(pat)
            whole = eng.vocoder(codes[2][:F], 0, out=spec)
            got, at = [], 0
            for j, n in enumerate(pat):
                last = j == len(pat) - 1
                got.append(st.push(codes[2][at:at + n], final=last))
                at += n
                assert st.frames == at and st.samples == eng.vocoder_num_samples(at, 0)
                assert st.out_samples == q3t.pcm_num_samples(eng.vocoder_num_samples(at, 0), rate, last)
                assert st.out_samples == sum(len(g) for g in got)
            g = np.concatenate(got)
            assert g.dtype == whole.dtype == R.DTYPES[fmt] and g.tobytes() == whole.tobytes(), (spec, pat)


def test_batched_push_gives_the_bytes_of_single_pushes(setup):
    """five streams, mixed specs and positions, three rounds; the groups are the plain batched push's, and each call
    makes exactly one conversion launch"""
    q3t, eng, codes, pcm = setup
    specs = [(8000, q3t.PCM_MULAW), (24000, q3t.PCM_S16), (44100, q3t.PCM_F32), (16000, q3t.PCM_S16), (8000, q3t.PCM_MULAW)]
    rounds = [[3, 1, 4, 4, 2], [4, 4, 4, 1, 7], [1, 2, 4, 4, 4]]
    first = [0, 5, 0, 2, 9]                                 # frames pushed singly before the batched rounds
    finals = [[False] * 5, [False, True, False, False, False], [True, False, True, True, True]]
    batch = [eng.vocoder_stream(F_ALL, out=s) for s in specs]
    single = [eng.vocoder_stream(F_ALL, out=s) for s in specs]
    plain = [eng.vocoder_stream(F_ALL) for _ in specs]
    at = list(first)
    for j, f in enumerate(first):
        if f:
            a, b = batch[j].push(codes[j][:f]), single[j].push(codes[j][:f])
            plain[j].push(codes[j][:f])
            assert a.tobytes() == b.tobytes()
    for r, (ns, fin) in enumerate(zip(rounds, finals)):
        live = [j for j in range(5) if not (r == 2 and j == 1)]        # stream 1 ended in round 1
        pieces = [codes[j][at[j]:at[j] + ns[j]] for j in live]
        before = q3t.lib().q3t_pcm_out_launches()
        outs = eng.vocoder_stream_push_batch([batch[j] for j in live], pieces, final=[fin[j] for j in live])
        assert q3t.lib().q3t_pcm_out_launches() == before + 1
        groups = eng.vocoder_stream_last_groups()
        eng.vocoder_stream_push_batch([plain[j] for j in live], pieces)
        assert groups == eng.vocoder_stream_last_groups()
        for j, o, p in zip(live, outs, pieces):
            alone = single[j].push(p, final=fin[j])
            assert o.dtype == alone.dtype and o.tobytes() == alone.tobytes(), (r, j)
            at[j] += ns[j]
            assert batch[j].frames == at[j] and batch[j].out_samples == single[j].out_samples
    # a finished stream refuses the next batched push, and nobody moves
    frames = [s.frames for s in batch]
    expect_error(q3t, lambda: eng.vocoder_stream_push_batch(batch[2:4], [codes[2][:1], codes[3][:1]]), "final", "stream 0")
    assert [s.frames for s in batch] == frames
    for s in batch + single + plain:
        s.close()


def test_a_final_push_of_no_frames_flushes_the_tail(setup):
    """the final delivery of a queue may be empty: single and batched, beside streams that push frames"""
    q3t, eng, codes, pcm = setup
    specs = [(8000, q3t.PCM_S16), (44100, q3t.PCM_MULAW), (24000, q3t.PCM_F32)]
    empty = np.zeros((0, 16), np.int32)
    for spec in specs:
        whole = eng.vocoder(codes[3][:20], 0, out=spec)
        with eng.vocoder_stream(F_ALL, out=spec) as st:
            got = [st.push(codes[3][:13]), st.push(codes[3][13:20]), st.push(empty, final=True)]
            assert st.frames == 20 and st.out_samples == len(whole)
            assert len(got[2]) == q3t.pcm_num_samples(st.samples, spec[0], True) - q3t.pcm_num_samples(st.samples, spec[0])
            assert np.concatenate(got).tobytes() == whole.tobytes(), spec
            expect_error(q3t, lambda: st.push(empty, final=True), "final")
    # batched: two streams flush while a third pushes frames, then a call in which every stream flushes
    sts = [eng.vocoder_stream(F_ALL, out=s) for s in specs]
    wholes = [eng.vocoder(codes[j][:12], 0, out=s) for j, s in enumerate(specs)]
    a = eng.vocoder_stream_push_batch(sts, [codes[0][:12], codes[1][:12], codes[2][:5]])
    groups = eng.vocoder_stream_last_groups()
    before = q3t.lib().q3t_pcm_out_launches()
    b = eng.vocoder_stream_push_batch(sts, [empty, empty, codes[2][5:12]], final=[True, True, False])
    assert q3t.lib().q3t_pcm_out_launches() == before + 1 and eng.vocoder_stream_last_groups() == 1 <= groups
    c = eng.vocoder_stream_push_batch(sts[2:], [empty], final=[True])
    assert eng.vocoder_stream_last_groups() == 0          # no stream pushed a frame: the stage alone ran
    assert np.concatenate([a[0], b[0]]).tobytes() == wholes[0].tobytes()
    assert np.concatenate([a[1], b[1]]).tobytes() == wholes[1].tobytes()
    assert np.concatenate([a[2], b[2], c[0]]).tobytes() == wholes[2].tobytes()
    # no frames and not final is still refused, and nobody moves
    fresh = eng.vocoder_stream(F_ALL, out=specs[0])
    expect_error(q3t, lambda: eng.vocoder_stream_push_batch([fresh], [empty]), "n_frames must be > 0")
    expect_error(q3t, lambda: fresh.push(empty), "n_frames must be > 0")
    assert fresh.frames == 0 and fresh.out_samples == 0
    for s_ in sts + [fresh]:
        s_.close()


def test_reset_gives_a_fresh_streams_pushes(setup):
    q3t, eng, codes, pcm = setup
    spec = (16000, q3t.PCM_S16)
    with eng.vocoder_stream(F_ALL, out=spec) as used, eng.vocoder_stream(F_ALL, out=spec) as fresh:
        used.push(codes[3][:9])
        used.push(codes[3][9:13], final=True)
        used.reset()
        assert (used.frames, used.samples, used.out_samples) == (0, 0, 0)
        for a, b, fin in ((0, 5, False), (5, 6, False), (6, 20, True)):
            x, y = used.push(codes[4][a:b], final=fin), fresh.push(codes[4][a:b], final=fin)
            assert x.tobytes() == y.tobytes() and len(x) > 0


# ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_stream_where_it_was(setup):
    q3t, eng, codes, pcm = setup
    lib = q3t.lib()
    spec = (12000, q3t.PCM_S16)
    whole = eng.vocoder(codes[0][:12], 0, out=spec)
    # rate 11025, format 3: one-shot and stream
    expect_error(q3t, lambda: eng.vocoder(codes[0], 0, out=(11025, q3t.PCM_S16)), "11025", "8000", "48000")
    expect_error(q3t, lambda: eng.vocoder(codes[0], 0, out=(8000, 3)), "format 3")
    st = eng.vocoder_stream(F_ALL)
    expect_error(q3t, lambda: st.set_output((11025, q3t.PCM_S16)), "11025", "22050")
    expect_error(q3t, lambda: st.set_output((8000, 3)), "format 3")
    assert st.out is None and st.out_samples == -1
    # an _out push without a spec
    buf = np.zeros(1 << 16, np.uint8)
    ns = C.c_int64(7)
    c5 = np.ascontiguousarray(codes[0][:5])
    assert lib.q3t_vocoder_stream_push_out(st.h, c5.ctypes.data, 5, 0, buf.ctypes.data, buf.nbytes, C.byref(ns)) != 0
    assert "no output spec" in lib.q3t_last_error().decode() and ns.value == 0 and st.frames == 0
    # the plain push still works on it, then set_output after a frame is refused and the plain stream goes on
    a = st.push(codes[0][:5])
    expect_error(q3t, lambda: st.set_output(spec), "zero frames")
    b = st.push(codes[0][5:12])
    assert np.concatenate([a, b]).tobytes() == pcm[0][:eng.vocoder_num_samples(12, 0)].tobytes()
    st.close()

    st = eng.vocoder_stream(F_ALL, out=spec)
    # a plain push on a stream with a spec
    f32 = np.zeros(1 << 16, np.float32)
    assert lib.q3t_vocoder_stream_push(st.h, c5.ctypes.data, 5, f32.ctypes.data, f32.size, C.byref(ns)) != 0
    assert "output spec" in lib.q3t_last_error().decode() and ns.value == 0
    assert (st.frames, st.samples, st.out_samples) == (0, 0, 0)
    # out_cap_bytes one byte short
    need = q3t.pcm_num_samples(eng.vocoder_num_samples(5, 0), 12000, False) * 2
    assert lib.q3t_vocoder_stream_push_out(st.h, c5.ctypes.data, 5, 0, buf.ctypes.data, need - 1, C.byref(ns)) != 0
    msg = lib.q3t_last_error().decode()
    assert "out_cap_bytes" in msg and str(need) in msg and ns.value == 0
    assert (st.frames, st.samples, st.out_samples) == (0, 0, 0)
    # the next good pushes are a fresh stream's
    a = st.push(codes[0][:5])
    assert a.nbytes == need
    b = st.push(codes[0][5:12], final=True)
    assert np.concatenate([a, b]).tobytes() == whole.tobytes()
    # a push after final
    state = (st.frames, st.samples, st.out_samples)
    expect_error(q3t, lambda: st.push(codes[0][12:13]), "final")
    assert (st.frames, st.samples, st.out_samples) == state
    st.reset()
    a = st.push(codes[0][:12], final=True)
    assert a.tobytes() == whole.tobytes()
    st.close()
    # the one-shot call's capacity check
    sp = q3t.PcmSpec(*spec)
    c12 = np.ascontiguousarray(codes[0][:12])
    assert lib.q3t_vocoder_decode_out(eng.h, c12, 12, 0, C.byref(sp), buf.ctypes.data, whole.nbytes - 1, C.byref(ns)) != 0
    assert "out_cap_bytes" in lib.q3t_last_error().decode()


def test_a_stream_that_never_had_a_spec_is_as_before(setup):
    q3t, eng, codes, pcm = setup
    with eng.vocoder_stream(F_ALL) as st:
        got = [st.push(codes[1][a:b]) for a, b in ((0, 7), (7, 8), (8, 40))]
        assert st.out_samples == -1
    assert np.concatenate(got).tobytes() == pcm[1].tobytes()
