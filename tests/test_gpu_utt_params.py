"""Per-utterance language, speaker, sampling and max_len in one batch or one queue (q3t_generate_utt /
q3t_generate_queue_utt; the per_utt argument of the Python wrapper).

The property under test: a mixed call gives each utterance, bit for bit, what a homogeneous call with that utterance's
values gives it at the same slot count.  Sampling is keyed by (seed, utterance index, frame, step) and no decode kernel
mixes slots, so the only thing a neighbour with other values may change is nothing.  No tolerance is involved.

  sampling mix     triples A (T 0.9, top-k 50, rep 1.05), B (greedy, rep 1.0), C (T 1.3, top-k 8, rep 1.2) round-robin
                   against the three homogeneous runs, through the queue and through generate(); the three runs must
                   differ from each other or the comparison shows nothing
  language/speaker five classes (language 2050 with / without a speaker, nothink with / without, language 2055 without):
                   prompts of 8, 9 and 10 rows in one admission batch (the ragged prefill) and in slots that are
                   refilled with a longer prompt than they held
  families         the mix at 2 slots (fused GEMV selection), 1 slot (the values go into the captured graphs' scalars),
                   16 slots (k_tkb / k_cpb) and on the 1.7B layout
  own max_len      n_frames[u] <= max_len[u], rows equal the uniform run's, no delivery beyond an utterance's cap
  identity         records copied from the call's parameters give the old entry points' codes
  errors           every validation failure: message, n_frames zero, the next valid call unchanged
Prompts of 5..12 text tokens at max_len 24 as in test_gpu_queue.py: EOS stops and max_len stops both occur.
"""
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu

NF = 24
A = dict(temperature=0.9, top_k=50, repetition_penalty=1.05)
B = dict(temperature=0.0, top_k=50, repetition_penalty=1.0)
Cc = dict(temperature=1.3, top_k=8, repetition_penalty=1.2)
TRIPLES = (A, B, Cc)


def _prompts(n, seed, cfg="full"):   # test_gpu_queue.py's
    base = prompt(cfg)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(5, 13))
        tail = [(t + 13 * i) % 900 + 20 for t in base[4:]]
        out.append(base[:4] + tail[:k - 4])
    return out


def _speakers(n, H):
    rng = np.random.default_rng(2)
    return [(rng.standard_normal(H) * 0.02).astype(np.float32) for _ in range(n)]


def _engine(cfg, slots, max_ctx=NF + 40):
    import q3t
    tts, _ = synth_dir(cfg)
    return q3t.Engine(tts, None, device=0, max_slots=slots, max_ctx=max_ctx)


@pytest.fixture(scope="module")
def eng4():
    eng = _engine("full", 4)
    yield eng
    eng.close()


def _n_differ(a, b):
    return sum(not np.array_equal(x, y) for x, y in zip(a, b))


def _check_sampling_mix(run, n_utt):
    """run(per_utt=None, **kw) -> list of codes.  Homogeneous runs under A, B, C, then the round-robin mix."""
    homo = [run(**t) for t in TRIPLES]
    for i, j in ((0, 1), (0, 2), (1, 2)):
        d = _n_differ(homo[i], homo[j])
        print(f"homogeneous runs {i} and {j} differ in {d} of {n_utt} utterances")
        assert 2 * d >= n_utt, (i, j, d)
    mixed = run(per_utt=[TRIPLES[u % 3] for u in range(n_utt)], **A)
    bad = [u for u in range(n_utt) if not np.array_equal(mixed[u], homo[u % 3][u])]
    assert not bad, (bad, [(len(mixed[u]), len(homo[u % 3][u])) for u in bad])
    return homo, mixed


# ---------------------------------------------------------------------------------------------- 1. sampling mix
def test_sampling_mix_queue(eng4):
    prompts = _prompts(8, 4)
    homo, _ = _check_sampling_mix(lambda **kw: eng4.generate_queue(prompts, max_len=NF, seed=123, **kw), 8)
    lens = [len(c) for c in homo[0]]
    assert 0 < min(lens) and max(lens) <= NF


def test_sampling_mix_generate(eng4):
    prompts = _prompts(4, 5)
    _check_sampling_mix(lambda **kw: eng4.generate(prompts, max_len=NF, seed=77, **kw), 4)


# ---------------------------------------------------------------------------------------------- 2. language / speaker
def test_language_and_speaker_mix(eng4):
    n_utt = 10
    prompts = _prompts(n_utt, 9)
    spk = _speakers(n_utt, eng4.cfg["hidden"])
    # (language, with speaker): prompts of 10, 9, 9, 9 and 8 rows
    classes = [(2050, True), (2050, False), (-1, True), (2055, False), (-1, False)]
    kw = dict(max_len=NF, seed=31, **A)
    homo = [eng4.generate_queue(prompts, speakers=spk if with_spk else None, language_id=lang, **kw)
            for lang, with_spk in classes]
    for i in range(len(classes)):
        for j in range(i + 1, len(classes)):
            assert _n_differ(homo[i], homo[j]) > 0, (classes[i], classes[j])
    rows = [len(eng4.prefill_embd(prompts[u], spk[u] if classes[u % 5][1] else None, language_id=classes[u % 5][0])[0])
            for u in range(n_utt)]
    assert set(rows) == {8, 9, 10}, rows
    # slot 0 holds utterance 0 (10 rows), then one of the later ones: refills with longer and shorter prompts both occur
    per_utt = [dict(language_id=classes[u % 5][0]) for u in range(n_utt)]
    mix_spk = [spk[u] if classes[u % 5][1] else None for u in range(n_utt)]
    mixed = eng4.generate_queue(prompts, speakers=mix_spk, per_utt=per_utt, **kw)
    bad = [u for u in range(n_utt) if not np.array_equal(mixed[u], homo[u % 5][u])]
    assert not bad, (bad, rows)
    # the streaming forms take the same arguments (speaker entries of None included)
    pieces = {u: [] for u in range(n_utt)}
    ret = eng4.generate_queue_stream(prompts, lambda es: [pieces[u].append(c) for u, c, _ in es] and None, interval=6,
                                     speakers=mix_spk, per_utt=per_utt, **kw)
    for u in range(n_utt):
        cat = np.concatenate(pieces[u]) if pieces[u] else np.zeros((0, 16), np.int32)
        assert np.array_equal(ret[u], mixed[u]) and np.array_equal(cat, mixed[u]), u
    g_stream = eng4.generate_stream(prompts[:4], lambda u, c: True, interval=6, speakers=mix_spk[:4], per_utt=per_utt[:4], **kw)
    # the same mix in lock-step: the first four utterances through generate()
    g_homo = [eng4.generate(prompts[:4], speakers=spk[:4] if with_spk else None, language_id=lang, **kw)
              for lang, with_spk in classes[:4]]
    g_mixed = eng4.generate(prompts[:4], speakers=mix_spk[:4], per_utt=per_utt[:4], **kw)
    bad = [u for u in range(4) if not np.array_equal(g_mixed[u], g_homo[u][u])]
    assert not bad, bad
    assert _n_differ(g_stream, g_mixed) == 0


# ---------------------------------------------------------------------------------------------- 3. families
def test_sampling_mix_two_slots():
    eng = _engine("full", 2)
    try:
        assert eng.decode_family(2) == 0   # the weight-streaming kernels with the fused selections
        prompts = _prompts(6, 6)
        _check_sampling_mix(lambda **kw: eng.generate_queue(prompts, max_len=NF, seed=5, **kw), 6)
        _check_sampling_mix(lambda **kw: eng.generate(prompts[:2], max_len=NF, seed=5, **kw), 2)
    finally:
        eng.close()


def test_sampling_mix_one_slot():
    """one slot: the utterance's values are baked into the captured graphs when it takes the slot.  Every utterance
    equals its row of the homogeneous one-slot queue; where an own one-utterance run is the same computation (utterance
    0, and the greedy ones, whose codes do not depend on the sampling key's utterance index) it equals that too."""
    eng = _engine("full", 1)
    try:
        prompts = _prompts(4, 7)
        kw = dict(max_len=NF, seed=9)
        homo, mixed = _check_sampling_mix(lambda **k: eng.generate_queue(prompts, **kw, **k), 4)
        for u in range(4):
            if u == 0 or TRIPLES[u % 3] is B:
                own = eng.generate_queue([prompts[u]], **kw, **TRIPLES[u % 3])[0]
                assert np.array_equal(mixed[u], own), u
                own = eng.generate([prompts[u]], per_utt=[TRIPLES[u % 3]], **kw)[0]
                assert np.array_equal(mixed[u], own), u
        assert eng.persist_status() in (0, -1)
    finally:
        eng.close()


def test_sampling_mix_sixteen_slots():
    eng = _engine("full", 16)
    try:
        assert eng.persist_kernels() & 48 == 48, "the batched persistent talker step / code-predictor frame are not in use"
        prompts = _prompts(24, 8)
        _check_sampling_mix(lambda **kw: eng.generate_queue(prompts, max_len=NF, seed=11, **kw), 24)
        assert eng.persist_status() == 0
    finally:
        eng.close()


def test_sampling_mix_tiny17():
    eng = _engine("tiny17", 4)
    try:
        assert eng.cfg["has_mtp"] == 1
        prompts = _prompts(8, 3, "tiny17")
        _check_sampling_mix(lambda **kw: eng.generate_queue(prompts, max_len=NF, seed=21, **kw), 8)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 4. own max_len
def test_own_max_len(eng4):
    n_utt = 8
    prompts = _prompts(n_utt, 12)
    caps = [(5, 24, 12, 1)[u % 4] for u in range(n_utt)]
    per_utt = [dict(max_len=c) for c in caps]
    kw = dict(max_len=NF, seed=41, force_frames=NF, **A)   # no EOS stop: every utterance reaches its cap
    uni = eng4.generate_queue(prompts, **kw)
    assert all(len(c) == NF for c in uni)
    own = eng4.generate_queue(prompts, per_utt=per_utt, **kw)
    for u in range(n_utt):
        assert len(own[u]) == caps[u], (u, len(own[u]), caps[u])
        assert np.array_equal(own[u], uni[u][:caps[u]]), u
    # with EOS stops: never more than the cap, and a prefix of the uniform run
    kw["force_frames"] = 0
    uni = eng4.generate_queue(prompts, **kw)
    own = eng4.generate_queue(prompts, per_utt=per_utt, **kw)
    for u in range(n_utt):
        assert len(own[u]) == min(caps[u], len(uni[u])), (u, len(own[u]), caps[u], len(uni[u]))
        assert np.array_equal(own[u], uni[u][:len(own[u])]), u
    # deliveries: no piece reaches beyond the utterance's own cap; their concatenation is what the call returns
    got = {u: [] for u in range(n_utt)}
    finals = {u: 0 for u in range(n_utt)}

    def on_batch(entries):
        for u, codes, final in entries:
            got[u].append(codes)
            finals[u] += final
            assert sum(len(c) for c in got[u]) <= caps[u], (u, caps[u])

    ret = eng4.generate_queue_stream(prompts, on_batch, interval=4, per_utt=per_utt, **kw)
    for u in range(n_utt):
        cat = np.concatenate(got[u]) if got[u] else np.zeros((0, 16), np.int32)
        assert finals[u] == 1 and np.array_equal(cat, ret[u]) and np.array_equal(ret[u], own[u]), u
    # lock-step: generate() and its frame callback
    g_uni = eng4.generate(prompts[:4], **kw)
    seen = {u: 0 for u in range(4)}

    def on_frames(u, codes):
        seen[u] += len(codes)
        assert seen[u] <= caps[u], (u, seen[u], caps[u])

    g_own = eng4.generate_stream(prompts[:4], on_frames, interval=4, per_utt=per_utt[:4], **kw)
    for u in range(4):
        assert len(g_own[u]) == min(caps[u], len(g_uni[u])) and np.array_equal(g_own[u], g_uni[u][:len(g_own[u])]), u
        assert seen[u] == len(g_own[u]), (u, seen[u])


# ---------------------------------------------------------------------------------------------- 5. identity
def test_records_from_the_call_equal_the_old_entry_points(eng4):
    n_utt = 8
    prompts = _prompts(n_utt, 15)
    spk = _speakers(n_utt, eng4.cfg["hidden"])
    for kw in (dict(max_len=NF, seed=3, **A), dict(max_len=NF, seed=3, language_id=-1, **Cc)):
        old = eng4.generate_queue(prompts, speakers=spk, **kw)
        new = eng4.generate_queue(prompts, speakers=spk, per_utt=[None] * n_utt, **kw)
        assert _n_differ(old, new) == 0
        old = eng4.generate(prompts[:4], speakers=spk[:4], **kw)
        new = eng4.generate(prompts[:4], speakers=spk[:4], per_utt=[None] * 4, **kw)
        assert _n_differ(old, new) == 0
        # alternating the entry points keeps both sets of captured graphs: the old one again, unchanged
        assert _n_differ(old, eng4.generate(prompts[:4], speakers=spk[:4], **kw)) == 0


# ---------------------------------------------------------------------------------------------- 6. errors
def test_validation_errors_leave_no_trace(eng4):
    import q3t
    n_utt = 6
    prompts = _prompts(n_utt, 17)
    kw = dict(max_len=NF, seed=8, **A)
    good = [dict(TRIPLES[u % 3], max_len=NF) for u in range(n_utt)]   # (the third case raises the call's max_len)
    before = eng4.generate_queue(prompts, per_utt=good, **kw)
    before_g = eng4.generate(prompts[:4], per_utt=good[:4], **kw)
    V = eng4.cfg["codec_vocab"]
    cases = [
        (dict(language_id=V), {}, "language id out of range"),
        (dict(max_len=NF + 1), {}, "max_len exceeds the call's max_len"),
        (dict(max_len=60), dict(max_len=60), "max_len exceeds the context reserved at ctx creation"),
        (dict(top_k=-1), {}, "top_k must be >= 0"),
        (dict(repetition_penalty=0.0), {}, "repetition_penalty must be finite and > 0"),
        (dict(repetition_penalty=-1.5), {}, "repetition_penalty must be finite and > 0"),
        (dict(repetition_penalty=float("nan")), {}, "repetition_penalty must be finite and > 0"),
        (dict(repetition_penalty=float("inf")), {}, "repetition_penalty must be finite and > 0"),
        (dict(temperature=float("nan")), {}, "temperature must be finite"),
        (dict(temperature=float("inf")), {}, "temperature must be finite"),
    ]
    for bad, call_kw, msg in cases:
        for where in (0, 3):
            per_utt = [dict(good[u], **bad) if u == where else good[u] for u in range(n_utt)]
            for fn, n in ((eng4.generate_queue, n_utt), (eng4.generate, 4)):
                with pytest.raises(q3t.Q3TError, match=f"utterance {where}: {msg}") as ei:
                    fn(prompts[:n], per_utt=per_utt[:n], **dict(kw, **call_kw))
                assert ei.value.n_frames == [0] * n, (bad, ei.value.n_frames)
    after = eng4.generate_queue(prompts, per_utt=good, **kw)
    assert _n_differ(before, after) == 0
    assert _n_differ(before_g, eng4.generate(prompts[:4], per_utt=good[:4], **kw)) == 0
