"""The vocoder stream (q3t_vocoder_stream_*, Engine.vocoder_stream): frames pushed in pieces, PCM BIT-identical to the
one-shot FULL decode of all frames (Engine.vocoder(codes, 0)), and within the vocoder's PCM tolerance of the CPU oracle.

Every pattern decodes a prefix of one fixed 140-frame code sequence per configuration, so the oracle runs once (on its
first 40 frames; the decoder is causal, so that decode is the head of every longer one)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle_py import Oracle
from q3t_testutil import REPO, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu
PCM_TOL = {"tiny": 6e-3, "full": 6e-3}   # tests/test_gpu_vocoder.py PCM_TOL (GPU vs oracle, max |dPCM|)
F_ALL, F_ORC = 140, 40

PATTERNS = [
    [1] * 16,                      # the halo filling up (H' < H), windows starting at frame 0
    [63, 1, 1, 1],                 # a key-chunk boundary crossed by single-row pushes: P = 63, 64, 65
    [31, 33, 2],                   # a query count that is no tile multiple, an unaligned P
    [70, 70],                      # one push spanning two key chunks, three chunks in total
    [7, 40, 1, 16, 33, 3, 40],     # mixed
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
    codes = _codes(F_ALL, 77)
    orc = Oracle(tts, tok)
    head = orc.vocoder(codes[:F_ORC], 0)
    orc.close()
    yield cfg, eng, codes, head
    eng.close()


def stream_decode(eng, st, codes, pattern):
    """push codes in the pattern's pieces; checks the sample bookkeeping after every push"""
    out, at = [], 0
    for n in pattern:
        before = st.samples
        pcm = st.push(codes[at:at + n])
        at += n
        assert st.frames == at
        assert st.samples == eng.vocoder_num_samples(at, 0)
        assert pcm.dtype == np.float32 and pcm.shape == (st.samples - before,)
        out.append(pcm)
    return np.concatenate(out)


@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: "-".join(map(str, p)) if len(p) < 8 else f"{p[0]}x{len(p)}")
def test_stream_is_bit_exact(setup, pattern):
    cfg, eng, codes, head = setup
    F = sum(pattern)
    assert F <= F_ALL
    want = eng.vocoder(codes[:F], 0)
    with eng.vocoder_stream(max_frames=F) as st:
        assert st.frames == 0 and st.samples == 0 and st.halo > 0
        got = stream_decode(eng, st, codes, pattern)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} samples differ, first at {bad[0]} (halo {st_halo(eng)})"
    n = min(got.size, head.size)
    err = float(np.abs(got[:n] - head[:n]).max())
    print(f"{cfg} {pattern}: stream vs oracle max|d|={err:.3e} over {n} samples")
    assert err < PCM_TOL[cfg]


def st_halo(eng):
    with eng.vocoder_stream(max_frames=64) as st:
        return st.halo


class halo_env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("Q3T_VOC_STREAM_HALO")
        os.environ["Q3T_VOC_STREAM_HALO"] = str(self.value)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("Q3T_VOC_STREAM_HALO", None)
        else:
            os.environ["Q3T_VOC_STREAM_HALO"] = self.old


def test_halo_sensitivity(setup):
    """a halo of 2 frames is too short: the second push differs; 4 frames more than derived change nothing.  So the
    bit-exact test above would notice a halo derived too short, and extra halo is harmless."""
    cfg, eng, codes, _ = setup
    want = eng.vocoder(codes[:40], 0)
    n20 = eng.vocoder_num_samples(20, 0)
    derived = st_halo(eng)
    assert derived > 2
    with halo_env(2):
        st = eng.vocoder_stream(max_frames=40)   # the knob is read at open
    with st:
        assert st.halo == 2
        a, b = st.push(codes[:20]), st.push(codes[20:40])
    assert np.array_equal(a, want[:n20])
    assert b.shape == want[n20:].shape and not np.array_equal(b, want[n20:])
    with halo_env(derived + 4):
        st = eng.vocoder_stream(max_frames=40)
    with st:
        assert st.halo == derived + 4
        got = np.concatenate([st.push(codes[:20]), st.push(codes[20:40])])
    assert np.array_equal(got, want)


def test_two_streams_and_one_shot_decodes_interleave(setup):
    cfg, eng, codes, _ = setup
    ca, cb = codes[:50], _codes(45, 5)
    other = [_codes(33, 6), _codes(9, 7)]
    want_a, want_b, want_o = eng.vocoder(ca, 0), eng.vocoder(cb, 0), [eng.vocoder(c, 0) for c in other]
    sa, sb = eng.vocoder_stream(max_frames=50), eng.vocoder_stream(max_frames=64)
    ga, gb = [], []
    ga.append(sa.push(ca[:13]))
    gb.append(sb.push(cb[:30]))
    assert np.array_equal(eng.vocoder(other[0], 0), want_o[0])
    ga.append(sa.push(ca[13:14]))
    for g, w in zip(eng.vocoder_batch(other, 0), want_o):
        assert np.array_equal(g, w)
    gb.append(sb.push(cb[30:45]))
    ga.append(sa.push(ca[14:50]))
    assert (sa.frames, sb.frames) == (50, 45)
    sa.close()
    sb.close()
    assert np.array_equal(np.concatenate(ga), want_a)
    assert np.array_equal(np.concatenate(gb), want_b)


def test_errors_leave_the_stream_unchanged(setup):
    import q3t
    cfg, eng, codes, _ = setup
    want = eng.vocoder(codes[:12], 0)
    with eng.vocoder_stream(max_frames=12) as st:
        out = [st.push(codes[:5])]
        state = (st.frames, st.samples)
        with pytest.raises(q3t.Q3TError, match="exceeds max_frames"):
            st.push(codes[5:13])                      # 5 + 8 > 12
        assert (st.frames, st.samples) == state
        with pytest.raises(q3t.Q3TError, match="n_frames must be > 0"):
            st.push(np.zeros((0, 16), np.int32))
        assert (st.frames, st.samples) == state
        # a short pcm_cap, through the raw call
        c = np.ascontiguousarray(codes[5:12])
        need = eng.vocoder_num_samples(12, 0) - st.samples
        pcm = np.full(need, 7.0, np.float32)
        ns = C.c_int64(-1)
        rc = q3t.lib().q3t_vocoder_stream_push(st.h, c.ctypes.data_as(C.c_void_p), 7, pcm.ctypes.data_as(C.c_void_p),
                                                need - 1, C.byref(ns))
        assert rc != 0 and "pcm_cap" in q3t.lib().q3t_last_error().decode()
        assert ns.value == 0 and (pcm == 7.0).all()
        assert (st.frames, st.samples) == state
        out.append(st.push(codes[5:12]))
        assert st.frames == 12
    assert np.array_equal(np.concatenate(out), want)
    with pytest.raises(q3t.Q3TError, match="closed"):
        st.push(codes[:1])


def test_premise_one_shot_decode_of_a_prefix_is_a_prefix(setup):
    """what the stream rests on, by name: the FULL decode of the first k frames is the head of the decode of more"""
    cfg, eng, codes, _ = setup
    whole = eng.vocoder(codes[:96], 0)
    for k in (1, 13, 64, 65):
        part = eng.vocoder(codes[:k], 0)
        assert part.shape == (eng.vocoder_num_samples(k, 0),)
        assert np.array_equal(part, whole[:part.size]), k
