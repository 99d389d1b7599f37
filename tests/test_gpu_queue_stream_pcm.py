"""Queue deliveries into the streaming vocoder: the shape a serving loop has.  The callback of
Engine.generate_queue_stream keeps one VocoderStream per live utterance, taken from a pool as large as the slot count
and reset() on reuse, and makes ONE vocoder_stream_push_batch per callback.  Every utterance's concatenated PCM must be
BIT-identical to Engine.vocoder(codes[u]); and at least one callback with two or more entries must have run the
convolution stack as one group (vocoder_stream_last_groups() == 1), which is what the tick shape of the deliveries is
for.  VocoderStream.reset() is also checked alone: a stream that is reset and pushed again equals a fresh one."""
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu
NF, INTERVAL, SLOTS, N_UTT = 48, 12, 4, 10


def _prompts(n, seed):   # test_gpu_queue.py::_prompts
    base = prompt("full")
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(5, 13))
        tail = [(t + 13 * i) % 900 + 20 for t in base[4:]]
        out.append(base[:4] + tail[:k - 4])
    return out


@pytest.fixture(scope="module")
def eng():
    import q3t
    tts, tok = synth_dir("full")
    e = q3t.Engine(tts, tok, device=0, max_slots=SLOTS, max_ctx=NF + 40)
    yield e
    e.close()


def test_pool_of_reset_streams_gives_the_one_shot_pcm(eng):
    prompts = _prompts(N_UTT, SLOTS)
    spk = [np.zeros(eng.cfg["hidden"], np.float32)] * N_UTT
    pool = [eng.vocoder_stream(max_frames=NF) for _ in range(SLOTS)]
    free, used, mine = list(pool), set(), {}
    pcm = {u: [] for u in range(N_UTT)}
    shared = []   # (entries, groups) of every callback with at least two pushes

    def on_batch(entries):
        for u, c, fin in entries:
            if u not in mine and u not in used:
                mine[u] = free.pop()
                mine[u].reset()
                used.add(u)
        push = [(u, c) for u, c, _ in entries if len(c)]
        if push:
            out = eng.vocoder_stream_push_batch([mine[u] for u, _ in push], [c for _, c in push])
            for (u, _), p in zip(push, out):
                pcm[u].append(p)
            if len(push) >= 2:
                shared.append((len(push), eng.vocoder_stream_last_groups()))
        for u, _, fin in entries:
            if fin:
                free.append(mine.pop(u))

    codes = eng.generate_queue_stream(prompts, on_batch, interval=INTERVAL, speakers=spk, max_len=NF, temperature=0.9,
                                      top_k=50, seed=123)
    assert len(free) == SLOTS and not mine and len(used) == N_UTT
    for u in range(N_UTT):
        want = eng.vocoder(codes[u], 0)
        got = np.concatenate(pcm[u])
        assert got.dtype == np.float32 and got.shape == want.shape, (u, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"utterance {u}: {bad.size} samples differ, first at {bad[0]}"
    print("callbacks with >= 2 pushes (pushes, groups):", shared)
    assert any(g == 1 for _, g in shared), shared
    for st in pool:
        st.close()


def test_reset_stream_equals_a_fresh_one(eng):
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 2048, size=(12, 16), dtype=np.int32)
    other = rng.integers(0, 2048, size=(12, 16), dtype=np.int32)
    st = eng.vocoder_stream(max_frames=16)
    st.push(codes[:7])
    st.push(codes[7:])
    assert st.frames == 12 and st.samples == eng.vocoder_num_samples(12, 0)
    st.reset()
    assert st.frames == 0 and st.samples == 0
    again = np.concatenate([st.push(codes[:4]), st.push(codes[4:])])
    fresh = eng.vocoder_stream(max_frames=16)
    want = np.concatenate([fresh.push(codes[:4]), fresh.push(codes[4:])])
    assert again.shape == want.shape == (eng.vocoder_num_samples(12, 0),)
    assert np.array_equal(again, want) and np.array_equal(again, eng.vocoder(codes, 0))
    assert st.frames == 12 and st.samples == fresh.samples
    st.reset()   # and with other frames: nothing of the earlier ones is left in the caches, tails or halos
    assert np.array_equal(np.concatenate([st.push(other[:4]), st.push(other[4:])]), eng.vocoder(other, 0))
    st.close()
    fresh.close()
