"""Batched vocoder stream pushes (q3t_vocoder_stream_push_batch, Engine.vocoder_stream_push_batch): one push on each of
many streams through shared launches.  Every stream's concatenated PCM must be BIT-identical to the one-shot FULL
decode of its own frames (Engine.vocoder(codes, 0)) -- the property tests/test_gpu_voc_stream.py holds single pushes
to -- whatever the other streams of the call are doing, and q3t_vocoder_stream_last_groups must show that the
convolution stack really ran once per group of equal windows and not once per stream.

Every stream has its own code sequence of at most 140 frames (its own seed); the oracle runs once per configuration,
on the first 40 frames of one stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle_py import Oracle
from q3t_testutil import REPO, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu
PCM_TOL = 6e-3   # tests/test_gpu_voc_stream.py PCM_TOL (GPU vs oracle, max |dPCM|)
F_ALL, F_ORC = 140, 40

# tests/test_gpu_voc_stream.py PATTERNS, here as five concurrent streams
PATTERNS = [
    [1] * 16,
    [63, 1, 1, 1],
    [31, 33, 2],
    [70, 70],
    [7, 40, 1, 16, 33, 3, 40],
]


def _codes(F, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2048, size=(F, 16), dtype=np.int32)


@pytest.fixture(scope="module", params=["tiny", "full"])
def setup(request):
    import q3t
    cfg = request.param
    tts, tok = synth_dir(cfg)
    eng = q3t.Engine(None, tok, device=0)
    codes = [_codes(F_ALL, 300 + j) for j in range(6)]
    want = [eng.vocoder(c, 0) for c in codes]     # the decoder is causal: a prefix's decode is a prefix of this
    for a in codes + want:
        a.setflags(write=False)
    orc = Oracle(tts, tok)
    head = orc.vocoder(codes[0][:F_ORC], 0)
    orc.close()
    yield cfg, eng, codes, want, head
    eng.close()


def check_state(eng, streams, at):
    for st, a in zip(streams, at):
        assert st.frames == a
        assert st.samples == eng.vocoder_num_samples(a, 0)


def assert_prefix(eng, got, want, F, tag):
    """got (list of pieces) is, bit for bit, the head of the one-shot decode"""
    g = np.concatenate(got) if got else np.zeros(0, np.float32)
    assert g.dtype == np.float32 and g.shape == (eng.vocoder_num_samples(F, 0),), tag
    bad = np.flatnonzero(g != want[:g.size])
    assert bad.size == 0, f"{tag}: {bad.size} samples differ, first at {bad[0]}"


def test_the_five_patterns_as_one_batch(setup):
    cfg, eng, codes, want, head = setup
    K = len(PATTERNS)
    streams = [eng.vocoder_stream(max_frames=sum(p)) for p in PATTERNS]
    got, at = [[] for _ in range(K)], [0] * K
    for r in range(max(len(p) for p in PATTERNS)):
        live = [j for j in range(K) if r < len(PATTERNS[j])]
        before = [streams[j].samples for j in live]
        pcm = eng.vocoder_stream_push_batch([streams[j] for j in live],
                                            [codes[j][at[j]:at[j] + PATTERNS[j][r]] for j in live])
        assert len(pcm) == len(live)
        for j, p, b in zip(live, pcm, before):
            at[j] += PATTERNS[j][r]
            assert p.dtype == np.float32 and p.shape == (streams[j].samples - b,)
            got[j].append(p)
        check_state(eng, streams, at)
        assert 1 <= eng.vocoder_stream_last_groups() <= len(live)
    for j in range(K):
        assert at[j] == sum(PATTERNS[j]) <= F_ALL
        assert_prefix(eng, got[j], want[j], at[j], f"{cfg} pattern {PATTERNS[j]}")
    for st in streams:
        st.close()
    g0 = np.concatenate(got[0])
    n = min(g0.size, head.size)
    err = float(np.abs(g0[:n] - head[:n]).max())
    print(f"{cfg}: batched stream 0 vs oracle max|d|={err:.3e} over {n} samples")
    assert n == eng.vocoder_num_samples(16, 0)   # stream 0 has 16 frames; the 40-frame head is checked below
    assert err < PCM_TOL
    # the first 40 frames of one stream against the oracle: stream 0's codes, pushed beside two other streams
    sa, sb, sc = (eng.vocoder_stream(max_frames=64) for _ in range(3))
    out = []
    for lo, hi in ((0, 7), (7, 20), (20, 40)):
        out.append(eng.vocoder_stream_push_batch([sb, sa, sc], [codes[1][lo:hi + 3], codes[0][lo:hi], codes[2][lo:lo + 1]])[1])
    for st in (sa, sb, sc):
        st.close()
    g = np.concatenate(out)
    assert g.shape == head.shape
    err = float(np.abs(g - head).max())
    print(f"{cfg}: 40 batched frames vs oracle max|d|={err:.3e}")
    assert err < PCM_TOL
    assert np.array_equal(g, want[0][:g.size])


STEADY_P = (12, 40, 63, 64, 100)


def steady(eng, codes):
    streams = [eng.vocoder_stream(max_frames=F_ALL) for _ in STEADY_P]
    got = [[st.push(codes[j][:P])] for j, (st, P) in enumerate(zip(streams, STEADY_P))]
    return streams, got, list(STEADY_P)


def batch_round(eng, streams, codes, got, at, ns, idx=None):
    idx = list(range(len(streams))) if idx is None else idx
    pcm = eng.vocoder_stream_push_batch([streams[j] for j in idx], [codes[j][at[j]:at[j] + n] for j, n in zip(idx, ns)])
    for j, n, p in zip(idx, ns, pcm):
        got[j].append(p)
        at[j] += n
    check_state(eng, streams, at)
    return eng.vocoder_stream_last_groups()


def test_steady_state_shares_every_launch(setup):
    cfg, eng, codes, want, _ = setup
    streams, got, at = steady(eng, codes)
    halo = streams[0].halo
    print(f"{cfg}: halo {halo}")
    assert 2 <= halo <= min(STEADY_P), "the steady-state positions must all lie at or past the halo"
    for _ in range(3):
        assert batch_round(eng, streams, codes, got, at, [4] * 5) == 1
    assert batch_round(eng, streams, codes, got, at, [4, 4, 7, 4, 4]) == 2
    # a fresh stream at P = 0 has a shorter window: one more group than the same round without it
    with_fresh = streams + [eng.vocoder_stream(max_frames=F_ALL)]
    got.append([])
    at.append(0)
    g_without = batch_round(eng, with_fresh, codes, got, at, [4] * 5, idx=[0, 1, 2, 3, 4])
    g_with = batch_round(eng, with_fresh, codes, got, at, [4] * 6)
    assert g_without == 1 and g_with == g_without + 1
    for j, st in enumerate(with_fresh):
        assert_prefix(eng, got[j], want[j], at[j], f"{cfg} steady stream {j}")
        st.close()


def test_batched_and_single_pushes_and_one_shot_decodes_interleave(setup):
    cfg, eng, codes, want, _ = setup
    streams, got, at = steady(eng, codes)
    other = _codes(33, 6)
    want_o = eng.vocoder(other, 0)
    for r, ns in enumerate(([4] * 5, [1, 9, 2, 30, 5], [12] * 5)):
        batch_round(eng, streams, codes, got, at, ns)
        j = r % 2 * 3                                   # a single push on stream 0, then on stream 3
        got[j].append(streams[j].push(codes[j][at[j]:at[j] + 5]))
        at[j] += 5
        check_state(eng, streams, at)
        assert np.array_equal(eng.vocoder(other, 0), want_o)
    batch_round(eng, streams, codes, got, at, [3, 3], idx=[4, 1])   # a subset, in another order
    for j, st in enumerate(streams):
        assert_prefix(eng, got[j], want[j], at[j], f"{cfg} interleaved stream {j}")
        st.close()


def test_errors_leave_every_stream_unchanged(setup):
    import q3t
    cfg, eng, codes, want, _ = setup
    tts, tok = synth_dir(cfg)
    eng2 = q3t.Engine(None, tok, device=0)
    foreign = eng2.vocoder_stream(max_frames=32)
    sa, sb, sc = eng.vocoder_stream(max_frames=40), eng.vocoder_stream(max_frames=40), eng.vocoder_stream(max_frames=24)
    streams = [sa, sb, sc]
    got = [[p] for p in eng.vocoder_stream_push_batch(streams, [codes[0][:5], codes[1][:11], codes[2][:20]])]
    at = [5, 11, 20]
    state = [(st.frames, st.samples) for st in streams]

    def unchanged():
        assert [(st.frames, st.samples) for st in streams] == state
        assert (foreign.frames, foreign.samples) == (0, 0)

    piece = lambda j, n: codes[j][at[j]:at[j] + n]
    with pytest.raises(q3t.Q3TError, match="given twice"):
        eng.vocoder_stream_push_batch([sa, sb, sa], [piece(0, 4), piece(1, 4), piece(0, 4)])
    unchanged()
    with pytest.raises(q3t.Q3TError, match="not an open stream of this decoder"):
        eng.vocoder_stream_push_batch([sa, foreign, sb], [piece(0, 4), codes[3][:4], piece(1, 4)])
    unchanged()
    with pytest.raises(q3t.Q3TError, match="n_frames must be > 0"):
        eng.vocoder_stream_push_batch([sa, sb, sc], [piece(0, 4), np.zeros((0, 16), np.int32), piece(2, 4)])
    unchanged()
    with pytest.raises(q3t.Q3TError, match="exceeds max_frames"):
        eng.vocoder_stream_push_batch([sa, sb, sc], [piece(0, 4), piece(1, 4), piece(2, 5)])   # 20 + 5 > 24
    unchanged()
    # a pcm_cap one sample short for one stream, through the raw call
    ns_new = [4, 4, 4]
    cs = [np.ascontiguousarray(piece(j, n)) for j, n in enumerate(ns_new)]
    need = [eng.vocoder_num_samples(at[j] + n, 0) - streams[j].samples for j, n in enumerate(ns_new)]
    pcm = [np.full(k, 7.0, np.float32) for k in need]
    harr = (C.c_void_p * 3)(*[st.h.value for st in streams])
    carr = (C.c_void_p * 3)(*[c.ctypes.data for c in cs])
    parr = (C.c_void_p * 3)(*[p.ctypes.data for p in pcm])
    nf = (C.c_int32 * 3)(*ns_new)
    cap = (C.c_int64 * 3)(need[0], need[1] - 1, need[2])
    ns = (C.c_int64 * 3)(-1, -1, -1)
    rc = q3t.lib().q3t_vocoder_stream_push_batch(harr, 3, carr, nf, parr, cap, ns)
    assert rc != 0 and "pcm_cap" in q3t.lib().q3t_last_error().decode()
    assert list(ns) == [0, 0, 0] and all((p == 7.0).all() for p in pcm)
    unchanged()
    # and a correct batched push afterwards is still bit-exact
    for j, p in enumerate(eng.vocoder_stream_push_batch(streams, [piece(j, 4) for j in range(3)])):
        got[j].append(p)
        at[j] += 4
    check_state(eng, streams, at)
    for j, st in enumerate(streams):
        assert_prefix(eng, got[j], want[j], at[j], f"{cfg} stream {j} after the errors")
        st.close()
    foreign.close()
    eng2.close()
