"""Ragged batched speaker encoder (SpeakerEncoder::encode_batch, q3t_speaker_encode_batch, Engine.encode_speakers):
clips of different lengths through shared launches, every row bit for bit the embedding of that clip encoded alone."""
import os
import sys

import numpy as np
import pytest

from oracle_py import Oracle
from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))

pytestmark = pytest.mark.gpu

SR = 24000
# mel frames per clip (n = 256 * T samples): the smallest legal clip and its neighbour, an odd length, both neighbours
# of the 128-row conv tile edge, and a segment that straddles tiles
FRAMES = [5, 6, 37, 127, 128, 129, 300]


def voice_like(n, seed=7):
    """seeded speech-like test signal of n samples (tests/test_speaker.py's): a gliding harmonic source,
    syllable-rate amplitude modulation, noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f0 = 140 + 30 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(np.sin(k * ph) / k for k in range(1, 12))
    x *= 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t) ** 2
    x += 0.02 * rng.standard_normal(len(t))
    return (0.3 * x / np.abs(x).max()).astype(np.float32)


@pytest.fixture(scope="module")
def eng():
    import q3t
    tts, _ = synth_dir("full")
    e = q3t.Engine(tts, None, device=0, max_slots=1, max_ctx=256)
    yield e
    e.close()


@pytest.fixture(scope="module")
def clips():
    return [voice_like(256 * t, seed=100 + t) for t in FRAMES]


@pytest.fixture(scope="module")
def alone(eng, clips):
    """each clip encoded alone: the reference of every bit comparison here (computed once, never changed)"""
    ref = [eng.encode_speaker(c) for c in clips]
    for r in ref:
        r.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def batch(eng, clips):
    emb, ok = eng.encode_speakers(clips)
    emb.setflags(write=False)
    return emb, ok


def launches():
    import q3t
    return q3t.lib().q3t_speaker_launches()


def test_rows_equal_single_encodes(eng, batch, alone):
    emb, ok = batch
    assert emb.shape == (len(FRAMES), eng.speaker_dim()) and ok.all()
    for i, t in enumerate(FRAMES):
        assert np.isfinite(emb[i]).all() and np.abs(emb[i]).max() > 0, t
        assert np.array_equal(emb[i], alone[i]), (t, np.abs(emb[i] - alone[i]).max())


def test_order_and_duplicates_do_not_change_a_row(eng, clips, batch, alone):
    emb, _ = batch
    rev, ok = eng.encode_speakers(clips[::-1])
    assert ok.all()
    dup, ok = eng.encode_speakers([c for c in clips for _ in range(2)])
    assert ok.all()
    n = len(clips)
    for i, t in enumerate(FRAMES):
        assert np.array_equal(rev[n - 1 - i], alone[i]), t
        assert np.array_equal(dup[2 * i], alone[i]) and np.array_equal(dup[2 * i + 1], alone[i]), t
        assert np.array_equal(rev[n - 1 - i], emb[i]) and np.array_equal(dup[2 * i], emb[i]), t


def test_batch_row_matches_oracle(eng, clips, batch):
    """the 300-frame row against the CPU oracle at tests/test_speaker.py's tolerance (every conv input is f16 on both
    sides, the summation order differs); the other rows inherit it through bit identity with the single encode"""
    emb, _ = batch
    tts, tok = synth_dir("full")
    o = Oracle(tts, tok)
    try:
        r = o.encode_speaker(clips[FRAMES.index(300)])
    finally:
        o.close()
    g = emb[FRAMES.index(300)]
    rel = np.abs(g - r).max() / np.abs(r).max()
    cos = float(g @ r / np.linalg.norm(g) / np.linalg.norm(r))
    print(f"rel {rel:.3g} cos {cos:.7f}")
    assert rel < 1e-2 and cos > 0.9999, (rel, cos)


def test_small_groups_give_the_same_bits(eng, clips, batch, monkeypatch):
    """Q3T_SPK_GROUP_ROWS=256 (read at each call): the seven clips (packed rows 13, 14, 45, 135, 136, 137, 308) split
    into several groups, and the 300-frame clip, longer than a group, runs alone"""
    emb, _ = batch
    monkeypatch.setenv("Q3T_SPK_GROUP_ROWS", "256")
    before = launches()
    small, ok = eng.encode_speakers(clips)
    grouped = launches() - before
    monkeypatch.delenv("Q3T_SPK_GROUP_ROWS")
    before = launches()
    again, _ = eng.encode_speakers(clips)
    one = launches() - before
    assert ok.all() and np.array_equal(small, emb) and np.array_equal(again, emb)
    # groups {5, 6, 37, 127}, {128}, {129}, {300}: four launch trains where the default makes one
    assert grouped == 4 * one, (grouped, one)


def test_launches_do_not_grow_with_the_clips(eng, clips):
    before = launches()
    eng.encode_speaker(clips[2])
    single = launches() - before
    before = launches()
    eng.encode_speakers(clips[:2])
    two = launches() - before
    before = launches()
    eng.encode_speakers(clips[:6])
    six = launches() - before
    print(f"launches: one encode_speaker {single}, batch of 2 {two}, batch of 6 {six}")
    assert single > 0 and two == six and two < 2 * single, (single, two, six)


def test_bad_clips(eng, clips, alone):
    tiny = np.zeros(1, np.float32)
    short = voice_like(256 * 4, seed=3)   # 4 mel frames: below the reflect pads' minimum of 5
    mixed = [clips[2], tiny, clips[4], short, clips[0]]
    emb, ok = eng.encode_speakers(mixed, strict=False)
    assert ok.tolist() == [True, False, True, False, True]
    assert not emb[1].any() and not emb[3].any()
    assert np.array_equal(emb[0], alone[2]) and np.array_equal(emb[2], alone[4]) and np.array_equal(emb[4], alone[0])
    with pytest.raises(RuntimeError, match=r"clip 1\b"):
        eng.encode_speakers(mixed)
    with pytest.raises(RuntimeError, match=r"clip 3\b"):
        eng.encode_speakers([clips[2], clips[3], clips[4], short])
    emb, ok = eng.encode_speakers([tiny, short], strict=False)
    assert not ok.any() and not emb.any()
    emb, ok = eng.encode_speakers([])
    assert emb.shape == (0, eng.speaker_dim()) and ok.shape == (0,)


def test_speaker_only_context(clips, alone):
    import q3t
    tts, _ = synth_dir("full")
    e = q3t.Engine.speaker_only(tts)
    try:
        emb, ok = e.encode_speakers([clips[3], clips[1]])
    finally:
        e.close()
    assert ok.all() and np.array_equal(emb[0], alone[3]) and np.array_equal(emb[1], alone[1])


def test_batch_row_drives_generation(eng, batch, alone):
    """identical floats in, identical codes out: asserted once, at 8 forced frames"""
    emb, _ = batch
    i = FRAMES.index(129)
    a = eng.generate([prompt("full")], speakers=[emb[i]], max_len=8, temperature=0.0, force_frames=8)[0]
    b = eng.generate([prompt("full")], speakers=[alone[i]], max_len=8, temperature=0.0, force_frames=8)[0]
    assert a.shape == (8, 16) and np.array_equal(a, b)
