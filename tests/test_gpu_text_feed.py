"""Incremental text input (q3t_generate_queue_text / Engine.generate_queue_text): an utterance fed its text while it
speaks gives, bit for bit, the codes of the same utterance given whole.

Every comparison is np.array_equal against generate_queue(per_utt=...) on the whole prompts, on the same engine, with
the same seed, slot count and records.  There is no tolerance.

Prompts: base[:4] + text + base[-5:] for the whole form, base[:4] + text[:h] for a head (6..20 text ids in 20..919),
config `full`, max_len 40, sampling triple A, force_frames per utterance = its trailing rows + 4 so that no utterance
ends before its text does.

  projection   project_text of 1, 2, 3, 5, 8, 9 and 33 ids in one call equals each id alone (the precondition of the feed
               path: a projected row does not depend on the rows that share the launch)
  fed ahead    4 slots, 8 utterances, 5 open: everything at the first ask; nothing is ever held
  one per tick interval 1: the text arrives exactly as fast as it is consumed
  starvation   three utterances withheld at frames 0, at a middle row, and at the row before the close (every id known,
               only the end missing), beside slots that keep running
  all starved  2 slots withheld at the same frame: the loop launches nothing meanwhile
  ramp         one utterance run to 90 frames, past 4 * n_tokens, after a close at row 6
  deliveries   the starvation schedule with a delivery callback
  families     1 slot (persistent one-slot kernels), 2 slots (fused GEMV selection), 16 slots (k_tkb / k_cpb), full17
  errors       a short head, no source, a fed id out of range, too many ids; the next valid call is unchanged
  cancel/abort a held utterance cancelled by the delivery callback; the text source aborting the call
"""
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu

NF = 40
A = dict(temperature=0.9, top_k=50, repetition_penalty=1.05)


def _texts(lens, seed):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.integers(20, 920, n)] for n in lens]


def _whole(texts, cfg="full"):
    base = prompt(cfg)
    return [base[:4] + t + base[-5:] for t in texts]


def _heads(texts, h, cfg="full"):
    base = prompt(cfg)
    return [base[:4] + t[:k] for t, k in zip(texts, h)]


def _per_utt(texts):
    return [dict(force_frames=len(t) + 1 + 4) for t in texts]


def _engine(cfg, slots, max_ctx=NF + 40):
    import q3t
    tts, _ = synth_dir(cfg)
    return q3t.Engine(tts, None, device=0, max_slots=slots, max_ctx=max_ctx)


@pytest.fixture(scope="module")
def eng4():
    eng = _engine("full", 4)
    yield eng
    eng.close()


class Source:
    """text_source scripted per utterance.  rest[u]: the ids beyond the head.  plan[u]:
         "all"        everything and the end at the first ask
         "tick"       one id per ask, the end with the last
         ("slow", c)  one id on every (c + 1)-th ask, nothing on the asks between, the end with the last id
         (F, c)       at the first ask the ids that make F rows known (all of them if F is the text's length), then nothing
                      for the first c asks at frames >= F, then the rest and the end"""

    def __init__(self, texts, h, plan):
        self.rest = {u: list(texts[u][h[u]:]) for u in plan}
        self.h = dict((u, h[u]) for u in plan)
        self.plan = plan
        self.calls = {u: 0 for u in plan}
        self.withheld = {u: 0 for u in plan}
        self.log = []

    def __call__(self, u, frames, ahead):
        self.log.append((u, frames, ahead))
        self.calls[u] += 1
        p, rest = self.plan[u], self.rest[u]
        if p == "all":
            assert self.calls[u] == 1, "asked again after the end"
            return rest, True
        if p == "tick":
            if not rest:
                return [], True
            return [rest.pop(0)], not rest
        if p[0] == "slow":
            if (self.calls[u] - 1) % (p[1] + 1) != 0:
                return [], False
            return [rest.pop(0)], not rest
        F, c = p
        if self.calls[u] == 1:
            n = F - self.h[u]
            out, self.rest[u] = rest[:n], rest[n:]
            return out, False
        if frames < F:
            return [], False
        assert frames == F and ahead == 0, (u, frames, ahead)   # it cannot run past the rows it knows
        if self.withheld[u] < c:
            self.withheld[u] += 1
            return [], False
        out, self.rest[u] = rest, []
        return out, True


def _ref(eng, texts, cfg="full", **kw):
    return eng.generate_queue(_whole(texts, cfg), per_utt=_per_utt(texts), max_len=NF, **A, **kw)


def _assert_equal(got, want):
    bad = [u for u in range(len(want)) if not np.array_equal(got[u], want[u])]
    assert not bad, (bad, [(len(got[u]), len(want[u])) for u in bad])


# ---------------------------------------------------------------------------------------------- B1
def test_projection_is_row_invariant(eng4):
    ids = _texts([33], 1)[0]
    alone = [eng4.project_text([t]) for t in ids]
    for n in (1, 2, 3, 5, 8, 9, 33):
        rows = eng4.project_text(ids[:n])
        bad = [i for i in range(n) if not np.array_equal(rows[i], alone[i][0])]
        print(f"project_text: {n} ids in one call, rows that differ from the id alone: {bad}")
        assert not bad, (n, bad)


# ---------------------------------------------------------------------------------------------- B3
LENS8 = [12, 14, 12, 20, 6, 9, 17, 7]
OPEN8 = [1, 1, 1, 0, 1, 0, 1, 0]
H8 = [0, 2, 4, 0, 1, 0, 3, 0]
SEED8 = 105   # utterance 0 stops at an EOS (frame 25), the others at max_len


@pytest.fixture(scope="module")
def case8(eng4):
    """the 8-utterance case most tests share: (texts, the whole-prompt run's codes, the prompts with heads for the open
    utterances); computed once and left unchanged"""
    texts = _texts(LENS8, 3)
    want = _ref(eng4, texts, seed=SEED8)
    lens = [len(c) for c in want]
    print("reference lengths:", lens)
    assert all(n >= len(t) + 5 or n == NF for n, t in zip(lens, texts))
    assert min(lens) < NF and max(lens) == NF   # EOS stops and max_len stops both occur
    prompts = [hd if o else w for hd, w, o in zip(_heads(texts, H8), _whole(texts), OPEN8)]
    return texts, want, prompts


def _run8(eng4, prompts, src, texts, **kw):
    return eng4.generate_queue_text(prompts, OPEN8, src, per_utt=_per_utt(texts), max_len=NF, seed=SEED8, **A, **kw)


def test_fed_ahead(eng4, case8):
    texts, want, prompts = case8
    h = H8
    src = Source(texts, h, {u: "all" for u in range(8) if OPEN8[u]})
    got, held = _run8(eng4, prompts, src, texts)
    _assert_equal(got, want)
    assert held == [0] * 8
    assert all(n == 1 for n in src.calls.values())
    # frames 0 and the rows the head gives at the first ask
    assert sorted(src.log) == sorted((u, 0, h[u]) for u in range(8) if OPEN8[u])
    # open == all zero: the plain queue
    got, held = eng4.generate_queue_text(_whole(texts), [0] * 8, None, per_utt=_per_utt(texts), max_len=NF, seed=SEED8, **A)
    _assert_equal(got, want)


# ---------------------------------------------------------------------------------------------- B4
def test_one_id_per_tick(eng4):
    texts = _texts([6, 11, 8, 15, 7, 10], 4)
    want = _ref(eng4, texts, seed=7)
    h = [0, 1, 2, 0, 1, 0]
    src = Source(texts, h, {u: "tick" for u in range(6)})
    got, held = eng4.generate_queue_text(_heads(texts, h), [1] * 6, src, interval=1, per_utt=_per_utt(texts), max_len=NF,
                                         seed=7, **A)
    _assert_equal(got, want)
    print("held:", held)
    assert held == [0] * 6   # a row ahead at every frame: never starved


# ---------------------------------------------------------------------------------------------- B5
STARVE = {0: (0, 3), 1: (5, 3), 2: (12, 3)}   # (frames value, asks withheld): before the first frame, mid text, before the close


def _starve_plan(n_utt, open_):
    return {u: STARVE.get(u, "all") for u in range(n_utt) if open_[u]}


def test_starvation(eng4, case8):
    texts, want, prompts = case8
    assert STARVE[2][0] == len(texts[2])   # every id known, only the end withheld
    # the three cannot be held at the same loop frame: they start together and each must run to its point first
    assert STARVE[1][0] >= STARVE[0][1] and STARVE[2][0] >= STARVE[1][0] + STARVE[1][1]
    src = Source(texts, H8, _starve_plan(8, OPEN8))
    got, held = _run8(eng4, prompts, src, texts, interval=4)
    _assert_equal(got, want)
    print("held:", held, "stats:", eng4.text_feed_stats())
    assert all(held[u] >= 1 for u in STARVE) and all(held[u] == 0 for u in range(8) if u not in STARVE)
    assert all(src.withheld[u] == STARVE[u][1] for u in STARVE)
    # utterance 3 (closed, 25 forced frames) runs beside every hold: the loop never stood still
    assert eng4.text_feed_stats()["idle_rounds"] == 0


# ---------------------------------------------------------------------------------------------- B6
def test_all_slots_starved_launch_nothing():
    eng = _engine("full", 2)
    try:
        texts = _texts([9, 10], 6)
        want = _ref(eng, texts, seed=5)
        h = [1, 2]
        runs = {}
        for c in (0, 3):
            src = Source(texts, h, {0: (4, c), 1: (4, c)})
            got, held = eng.generate_queue_text(_heads(texts, h), [1, 1], src, interval=4, per_utt=_per_utt(texts),
                                                max_len=NF, seed=5, **A)
            _assert_equal(got, want)
            runs[c] = (held, eng.text_feed_stats())
            print(c, runs[c])
        assert runs[3][0] == [1, 1]
        assert runs[3][1]["idle_rounds"] == 3          # one per withheld ask: both slots held, nothing launched
        assert runs[3][1]["graph_launches"] == runs[0][1]["graph_launches"]
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- B7
def test_ramp_after_the_close():
    eng = _engine("full", 1, max_ctx=96 + 40)
    try:
        texts = _texts([6], 8)
        pu = [dict(force_frames=90)]
        want = eng.generate_queue(_whole(texts), per_utt=pu, max_len=96, seed=3, **A)
        assert len(want[0]) >= 90 and 4 * (4 + 6 + 5) == 60   # frames past expected = 60 run under the ramp
        src = Source(texts, [0], {0: "tick"})   # one id per ask
        got, held = eng.generate_queue_text(_heads(texts, [0]), [1], src, interval=2, per_utt=pu, max_len=96, seed=3, **A)
        _assert_equal(got, want)
        src = Source(texts, [0], {0: ("slow", 1)})
        got, held = eng.generate_queue_text(_heads(texts, [0]), [1], src, interval=2, per_utt=pu, max_len=96, seed=3, **A)
        _assert_equal(got, want)
        print("held:", held, eng.text_feed_stats())
        assert held[0] >= 1   # every id comes one ask late: the slot starves on the way to the close
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- B8
def test_deliveries(eng4, case8):
    texts, want, prompts = case8
    src = Source(texts, H8, _starve_plan(8, OPEN8))
    pieces = {u: [] for u in range(8)}

    def on_batch(entries):
        assert [e[0] for e in entries] == sorted(e[0] for e in entries)
        for u, codes, final in entries:
            pieces[u].append((codes, final))

    interval = 6
    got, held = _run8(eng4, prompts, src, texts, on_batch=on_batch, interval=interval)
    _assert_equal(got, want)
    assert all(held[u] >= 1 for u in STARVE)
    for u in range(8):
        ps = pieces[u]
        assert [f for _, f in ps].count(True) == 1 and ps[-1][1], u
        assert all(len(c) > 0 for c, f in ps if not f), u
        assert all(len(c) <= interval for c, _ in ps), u
        assert np.array_equal(np.concatenate([c for c, _ in ps]), got[u]), u
        if not OPEN8[u]:
            assert all(len(c) == interval for c, _ in ps[1:-1]), (u, [len(c) for c, _ in ps])


# ---------------------------------------------------------------------------------------------- B9
@pytest.mark.parametrize("cfg,slots,n_utt", [("full", 1, 4), ("full", 2, 4), ("full", 16, 16), ("full17", 4, 4)])
def test_families(cfg, slots, n_utt):
    eng = _engine(cfg, slots)
    try:
        if slots == 1:
            assert eng.persist_status() == 0 and eng.persist_kernels() & 5 == 5, eng.persist_kernels()
        if slots == 2:
            assert eng.decode_family(2) == 0
        if slots == 16:
            assert eng.persist_kernels() & 48 == 48, "the batched persistent talker step / code-predictor frame are not in use"
            assert eng.decode_family(16) == 2
        if cfg == "full17":
            assert eng.cfg["has_mtp"] == 1
        lens = (LENS8 + [8, 13, 6, 16, 10, 7, 19, 11])[:n_utt]
        open_ = ([1, 1, 1, 0] + [1, 0] * 6)[:n_utt]
        h = (H8 + [1, 0, 2, 0, 0, 0, 3, 0])[:n_utt]
        texts = _texts(lens, 3)
        want = _ref(eng, texts, cfg, seed=31)
        prompts = [hd if o else w for hd, w, o in zip(_heads(texts, h, cfg), _whole(texts, cfg), open_)]
        src = Source(texts, h, _starve_plan(n_utt, open_))
        got, held = eng.generate_queue_text(prompts, open_, src, interval=4, per_utt=_per_utt(texts), max_len=NF, seed=31, **A)
        _assert_equal(got, want)
        print("held:", held, eng.text_feed_stats())
        assert all(held[u] >= 1 for u in STARVE) and all(held[u] == 0 for u in range(n_utt) if u not in STARVE)
        if slots in (1, 16):
            assert eng.persist_status() == 0
    finally:
        eng.close()


def _env_engine(env, cfg, slots, max_ctx=NF + 40):   # test_gpu_concurrency.py's
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _engine(cfg, slots, max_ctx)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def test_fallback_rerun_replays_the_fed_text():
    """a hand-off fault flagged on the 21st persistent launch of a one-slot queue (the context's test hook): the re-run
    on the launch-per-op graphs replays what the source gave and asks only for what it had not: every id is given once
    (the scripted source raises if asked for more), the codes are those of a launch-per-op context"""
    ref = _env_engine({"Q3T_PERSIST": "0", "Q3T_CP_FUSED_ATTN": "0"}, "full", 1)
    flt = _env_engine({"Q3T_PERSIST_FAULT_AT": "21"}, "full", 1)
    try:
        assert flt.persist_status() == 0
        texts = _texts([12, 9, 7], 11)
        want = _ref(ref, texts, seed=13)
        h = [0, 2, 1]
        src = Source(texts, h, {0: (3, 2), 1: "all", 2: "tick"})
        got, held = flt.generate_queue_text(_heads(texts, h), [1, 1, 1], src, interval=4, per_utt=_per_utt(texts),
                                            max_len=NF, seed=13, **A)
        assert flt.persist_status() == 2, "the injected fault did not trigger the fallback"
        _assert_equal(got, want)
        print("held:", held, "asks:", src.calls)
        # nothing was asked for twice: one ask for the utterance fed ahead, one per id for the one fed id by id
        assert src.calls[1] == 1 and src.calls[2] == len(texts[2]) - h[2] and not src.rest[0] and not src.rest[2]
    finally:
        ref.close()
        flt.close()


# ---------------------------------------------------------------------------------------------- B10
def test_errors(eng4):
    import q3t
    texts = _texts([8, 9, 10], 9)
    kw = dict(per_utt=_per_utt(texts), max_len=NF, seed=17, **A)
    before = eng4.generate_queue(_whole(texts), **kw)
    heads = _heads(texts, [1, 1, 1])
    open_ = [0, 1, 0]
    prompts = [_whole(texts)[0], heads[1], _whole(texts)[2]]
    tv = eng4.cfg["text_vocab"]

    def expect(msg, prompts, src, open_=open_):
        with pytest.raises(q3t.Q3TError) as e:
            eng4.generate_queue_text(prompts, open_, src, interval=4, **kw)
        print(e.value)
        assert "utterance 1" in str(e.value) and msg in str(e.value), str(e.value)
        _assert_equal(eng4.generate_queue(_whole(texts), **kw), before)

    expect("at least 4", [prompts[0], heads[1][:3], prompts[2]], lambda u, f, a: ([], True))
    expect("callback", prompts, None)
    expect("out of range", [prompts[0], heads[1][:3] + [tv], prompts[2]], lambda u, f, a: ([], True))
    expect("out of range", prompts, lambda u, f, a: ([30, tv], True))
    expect("trailing-text buffer", prompts, lambda u, f, a: ([25] * 600, False))
    # fed in two halves, each within the buffer, together beyond it
    expect("trailing-text buffer", prompts, lambda u, f, a: ([25] * 300, False))


# ---------------------------------------------------------------------------------------------- B11
def test_cancel_a_held_utterance(eng4, case8):
    """utterance 1 starves for good at frames 5; once its first 5 frames are handed out the delivery callback cancels it.
    Its slot is refilled and every other utterance has the codes of the whole-prompt run."""
    texts, want, prompts = case8
    plan = {u: "all" for u in range(8) if OPEN8[u]}
    plan[1] = (5, 10 ** 9)
    src = Source(texts, H8, plan)
    seen = {u: 0 for u in range(8)}

    def on_batch(entries):
        stop = []
        for u, codes, final in entries:
            seen[u] += len(codes)
            if u == 1 and seen[1] >= 5:
                stop.append(1)
        return stop

    got, held = _run8(eng4, prompts, src, texts, on_batch=on_batch, interval=3)
    assert held[1] == 1 and len(got[1]) == 5 and np.array_equal(got[1], want[1][:5])
    for u in range(8):
        if u != 1:
            assert np.array_equal(got[u], want[u]), u


def test_text_source_aborts(eng4, case8):
    texts, want, prompts = case8
    inner = Source(texts, H8, {u: "all" for u in range(8) if OPEN8[u]})
    inner.plan[2] = (6, 10 ** 9)
    delivered = {u: 0 for u in range(8)}

    def src(u, frames, ahead):
        if u == 2 and inner.withheld[2] >= 4:
            return False
        return inner(u, frames, ahead)

    def on_batch(entries):
        for u, codes, final in entries:
            delivered[u] += len(codes)

    got, held = _run8(eng4, prompts, src, texts, on_batch=on_batch, interval=3)
    assert [len(c) for c in got] == [delivered[u] for u in range(8)]
    assert sum(delivered.values()) > 0 and len(got[2]) <= 6
    for u in range(8):
        assert np.array_equal(got[u], want[u][:len(got[u])]), u
    # the context is as any call leaves it
    _assert_equal(_ref(eng4, texts, seed=SEED8), want)
