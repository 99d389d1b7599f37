"""The open queue (q3t_generate_queue_open; Engine.generate_queue_open): utterances are admitted while continuous
batching runs.

The property everything rests on: an utterance that arrives with key k, record r, speaker s and tokens t gets, bit for
bit and in length, the codes generate_queue(per_utt=...) returns for index k of a closed call at the same slots, seed and
max_len in which utterance k has (t, s, r) -- whenever it arrived, whatever else ran, whichever slot it took.  No
tolerance is involved.  Arrivals are scripted against the loop's own progress (the source counts its asks and the
deliveries seen), never against wall time.  The `full` synthetic model at max_len 24 with the prompts of
test_gpu_utt_params.py (5..12 text tokens): EOS stops and max_len stops both occur.

  equality   12 utterances through 4 slots, 3 at the start, then ones and twos; sampling triples A / B / C round-robin and
             the five language / speaker classes (prompts of 8, 9 and 10 rows in one admission batch); the delivery contract
  keys       the same utterances in reverse order with key = original index: the same codes per key
  overlap    a newcomer is handed over while a long utterance runs and is heard before that one ends; once everything has
             ended the source is asked with idle = 1, hands one more over, and closes
  families   1 slot (the persistent one-slot kernels, the triple changing between utterances), 2 slots, 16 slots (k_tkb /
             k_cpb), the 1.7B layout at 4 slots
  control    max_active, cancel, abort by the arrival callback
  errors     more than room, every bad record (check_utt agrees), null callback / bad interval; the next valid call unchanged
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu

NF, INTERVAL = 24, 4
A = dict(temperature=0.9, top_k=50, repetition_penalty=1.05)
B = dict(temperature=0.0, top_k=50, repetition_penalty=1.0)
Cc = dict(temperature=1.3, top_k=8, repetition_penalty=1.2)
TRIPLES = (A, B, Cc)
# (language, with speaker): prompts of 10, 9, 8, 9 and 9 rows
CLASSES = [(2050, True), (2050, False), (-1, False), (-1, True), (2055, False)]


def _prompts(n, seed, cfg="full"):   # test_gpu_utt_params.py's
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


class Run:
    """One open call.  script(run, next_id, room, running, idle) -> (items, closed) | False is the source; the run records
    every ask and every delivery, and checks what must hold at each: ids in increasing order within a delivery, nothing
    after an utterance's final delivery, room and running within the slot count."""

    def __init__(self, eng, S, script, max_active=0, cancel=(), **params):
        self.asks, self.log, self.pieces, self.finals = [], [], {}, {}
        self.events = []   # ("ask", index) and ("deliver", id, n, final) in the order they happened
        self.cancelled = set()

        def source(next_id, room, running, idle):
            assert 0 < room <= S and 0 <= running < S and idle == (running == 0), (room, running, idle)
            assert next_id == sum(a[4] for a in self.asks)
            r = script(self, next_id, room, running, idle)
            n = 0 if r is False or r is None else len(r[0])
            self.events.append(("ask", len(self.asks)))
            self.asks.append((next_id, room, running, idle, min(n, room)))
            return r

        def on_batch(entries):
            ids = [e[0] for e in entries]
            assert ids == sorted(set(ids)) and ids, ids
            stop = []
            for u, c, fin in entries:
                assert not self.finals.get(u) and u not in self.cancelled, u
                self.pieces.setdefault(u, []).append(c)
                self.finals[u] = self.finals.get(u, 0) + int(fin)
                self.log.append((u, c, fin))
                self.events.append(("deliver", u, len(c), fin))
                if u in cancel and not fin:
                    stop.append(u)
                    self.cancelled.add(u)
            return stop or None

        self.n_arrived, self.n_finished = eng.generate_queue_open(source, on_batch, interval=INTERVAL, slots=S,
                                                                  max_active=max_active, **params)

    def cat(self, u):
        p = self.pieces.get(u, [])
        return np.concatenate(p) if p else np.zeros((0, 16), np.int32)

    def deliveries_of(self, u):
        return sum(1 for e in self.log if e[0] == u)


def check_contract(run, lengths, ids):
    """test_gpu_queue_stream.py's contract, per id: exactly one final delivery, the last; a non-final one has 1..interval
    frames, the final one 0..interval; one that is not the first and leaves the utterance unfinished has exactly `interval`"""
    for u in ids:
        d = [(c, fin) for v, c, fin in run.log if v == u]
        assert d and [fin for _, fin in d].count(True) == 1 and d[-1][1], (u, [(len(c), fin) for c, fin in d])
        got = 0
        for i, (c, fin) in enumerate(d):
            n = len(c)
            assert (0 if fin else 1) <= n <= INTERVAL, (u, i, n, fin)
            got += n
            if i > 0 and got < lengths[u]:
                assert n == INTERVAL, (u, i, n, got, lengths[u])


def in_order(items, first, later):
    """a source that hands `first` items at the first ask, then later[i % len(later)] at each further ask, in order"""
    state = {"next": 0, "ask": 0}

    def script(run, next_id, room, running, idle):
        want = first if state["ask"] == 0 else later[(state["ask"] - 1) % len(later)]
        state["ask"] += 1
        n = min(want, room, len(items) - state["next"])
        out = items[state["next"]:state["next"] + n]
        state["next"] += n
        return out, state["next"] == len(items)

    return script


class Case:
    """12 utterances with the triples and the classes round-robin, and their closed run at 4 slots (computed once)"""

    def __init__(self):
        self.eng = _engine("full", 4)
        self.n = 12
        self.prompts = _prompts(self.n, 1)
        spk = _speakers(self.n, self.eng.cfg["hidden"])
        self.spk = [spk[u] if CLASSES[u % 5][1] else None for u in range(self.n)]
        self.per_utt = [dict(TRIPLES[u % 3], language_id=CLASSES[u % 5][0]) for u in range(self.n)]
        self.kw = dict(max_len=NF, seed=7)   # (with these prompts: one EOS stop, eleven max_len stops)
        self.ref = self.eng.generate_queue(self.prompts, speakers=self.spk, per_utt=self.per_utt, **self.kw)
        self.lens = [len(c) for c in self.ref]

    def item(self, u, **more):
        return dict(prompt=self.prompts[u], speaker=self.spk[u], **dict(self.per_utt[u], **more))


@pytest.fixture(scope="module")
def case():
    c = Case()
    yield c
    c.eng.close()


# ------------------------------------------------------------------------------------------------- 1. equality
def test_arrivals_equal_the_closed_queue(case):
    eng = case.eng
    print("closed lengths", case.lens)
    assert any(n < NF for n in case.lens) and any(n == NF for n in case.lens), f"need EOS stops and max_len stops: {case.lens}"
    rows = [len(eng.prefill_embd(case.prompts[u], case.spk[u], language_id=CLASSES[u % 5][0])[0]) for u in range(3)]
    assert rows == [10, 9, 8], rows   # the first admission batch packs prompts of three lengths
    run = Run(eng, 4, in_order([case.item(u) for u in range(case.n)], 3, (1, 2)), **case.kw)
    assert (run.n_arrived, run.n_finished) == (case.n, case.n)
    assert run.asks[0][:4] == (0, 4, 0, True) and run.asks[0][4] == 3
    assert {a[4] for a in run.asks[1:]} >= {1, 2}, [a[4] for a in run.asks]
    check_contract(run, case.lens, range(case.n))
    for u in range(case.n):
        assert np.array_equal(run.cat(u), case.ref[u]), (u, len(run.cat(u)), case.lens[u])
    # the same call again on the same context, and the closed call after it: nothing lingers
    again = Run(eng, 4, in_order([case.item(u) for u in range(case.n)], 3, (1, 2)), **case.kw)
    assert all(np.array_equal(again.cat(u), case.ref[u]) for u in range(case.n))
    after = eng.generate_queue(case.prompts, speakers=case.spk, per_utt=case.per_utt, **case.kw)
    assert all(np.array_equal(after[u], case.ref[u]) for u in range(case.n))


# ------------------------------------------------------------------------------------------------- 2. keys
def test_codes_follow_the_key_not_the_arrival_order(case):
    items = [case.item(u, key=u) for u in reversed(range(case.n))]
    run = Run(case.eng, 4, in_order(items, 3, (2, 1)), **case.kw)
    assert run.n_arrived == case.n
    for i, u in enumerate(reversed(range(case.n))):   # id i carries key u
        assert np.array_equal(run.cat(i), case.ref[u]), (i, u, len(run.cat(i)), case.lens[u])
    check_contract(run, {i: case.lens[u] for i, u in enumerate(reversed(range(case.n)))}, range(case.n))


# ------------------------------------------------------------------------------------------------- 3. overlap, emptiness
def test_a_newcomer_is_heard_while_the_queue_runs_and_after_it_went_empty(case):
    eng = case.eng
    prompts = case.prompts[:3]
    per_utt = [dict(A, force_frames=NF, max_len=NF), dict(A), dict(Cc)]
    # the closed call at the same slot count: a fourth utterance makes it a 4-slot queue (the kernel family follows
    # min(slots, utterances))
    ref = eng.generate_queue(case.prompts[:4], per_utt=per_utt + [dict(A)], **case.kw)[:3]
    assert len(ref[0]) == NF
    handed = []

    def script(run, next_id, room, running, idle):
        if not handed:
            handed.append(0)
            return [dict(prompt=prompts[0], **per_utt[0])], False
        if handed == [0]:
            # the first ask after the first delivery of utterance 0 (it is running: the ask cannot be the idle one)
            if run.deliveries_of(0) >= 1:
                assert not idle and running == 1
                handed.append(1)
                return [dict(prompt=prompts[1], **per_utt[1])], False
            return [], False
        if handed == [0, 1]:
            if not idle:
                return [], False
            # nothing is busy: everything accepted so far has had its final delivery
            assert run.finals.get(0) == 1 and run.finals.get(1) == 1, run.finals
            handed.append(2)
            return [dict(prompt=prompts[2], **per_utt[2])], False
        return [], True   # the ask after that one closes

    run = Run(eng, 4, script, **case.kw)
    assert handed == [0, 1, 2] and (run.n_arrived, run.n_finished) == (3, 3)
    order = [(e[1], e[3]) for e in run.events if e[0] == "deliver"]
    assert order.index((1, False)) < order.index((0, True)), order   # 1 was heard before 0 ended
    assert run.asks[-1][2] == 1 and not run.asks[-1][3]              # the closing ask: utterance 2 was running
    idle_asks = [i for i, a in enumerate(run.asks) if a[3]]
    assert len(idle_asks) == 2 and idle_asks[0] == 0, idle_asks      # the start, and once after the queue went empty
    for u in range(3):
        assert np.array_equal(run.cat(u), ref[u]), (u, len(run.cat(u)), len(ref[u]))
    check_contract(run, [len(c) for c in ref], range(3))


# ------------------------------------------------------------------------------------------------- 4. families
@pytest.mark.parametrize("cfg,slots,n_utt", [("full", 1, 4), ("full", 2, 6), ("full", 16, 20), ("tiny17", 4, 8)],
                         ids=["1slot", "2slots", "16slots", "tiny17"])
def test_families(cfg, slots, n_utt):
    eng = _engine(cfg, slots)
    try:
        if slots == 16:
            assert eng.persist_kernels() & 48 == 48, "the batched persistent talker step / code-predictor frame are not in use"
        if slots == 1:
            assert eng.persist_kernels() & 15, "the one-slot persistent kernels are not in use"
        prompts = _prompts(n_utt, 7 + slots, cfg)
        per_utt = [TRIPLES[u % 3] for u in range(n_utt)]
        kw = dict(max_len=NF, seed=9)
        ref = eng.generate_queue(prompts, per_utt=per_utt, **kw)
        items = [dict(prompt=prompts[u], **per_utt[u]) for u in range(n_utt)]
        run = Run(eng, slots, in_order(items, max(1, slots // 2), (1, 2, 3)), **kw)
        assert (run.n_arrived, run.n_finished) == (n_utt, n_utt)
        for u in range(n_utt):
            assert np.array_equal(run.cat(u), ref[u]), (u, len(run.cat(u)), len(ref[u]))
        check_contract(run, [len(c) for c in ref], range(n_utt))
        if slots == 16:
            assert eng.persist_status() == 0
        if slots == 1:
            assert eng.persist_status() in (0, -1)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- 5. control
def test_max_active(case):
    run = Run(case.eng, 4, in_order([case.item(u) for u in range(case.n)], 4, (4,)), max_active=2, **case.kw)
    assert all(a[2] <= 2 and a[1] <= 2 for a in run.asks), run.asks
    assert max(a[4] for a in run.asks) == 2 and run.n_finished == case.n
    for u in range(case.n):
        assert np.array_equal(run.cat(u), case.ref[u]), u


def test_cancel_leaves_the_others_alone(case):
    victim = next(u for u in range(8) if case.lens[u] > 2 * INTERVAL)
    run = Run(case.eng, 4, in_order([case.item(u) for u in range(case.n)], 3, (1, 2)), cancel={victim}, **case.kw)
    assert run.cancelled == {victim} and run.finals[victim] == 0
    got = run.cat(victim)
    assert 0 < len(got) < case.lens[victim] and np.array_equal(got, case.ref[victim][:len(got)])
    for u in range(case.n):
        if u != victim:
            assert np.array_equal(run.cat(u), case.ref[u]) and run.finals[u] == 1, u
    # its slot went to a later arrival: every utterance arrived and ended although the victim never finished
    assert (run.n_arrived, run.n_finished) == (case.n, case.n)
    later = [e for e in run.events[run.events.index(("deliver", victim, len(run.pieces[victim][0]), False)):] if e[0] == "ask"]
    assert later and any(run.asks[e[1]][4] > 0 for e in later)


def test_abort_by_the_source(case):
    items = [case.item(u) for u in range(case.n)]
    inner = in_order(items, 3, (1, 2))

    def script(run, next_id, room, running, idle):
        if len(run.log) >= 6:
            return False
        return inner(run, next_id, room, running, idle)

    run = Run(case.eng, 4, script, **case.kw)   # returns: Q3T_OK
    finals = sum(run.finals.values())
    assert 0 < run.n_arrived < case.n and run.n_finished == finals <= run.n_arrived
    for u in run.pieces:   # what was handed out is a prefix of the utterance
        got = run.cat(u)
        assert np.array_equal(got, case.ref[u][:len(got)]), u
    after = case.eng.generate_queue(case.prompts, speakers=case.spk, per_utt=case.per_utt, **case.kw)
    assert all(np.array_equal(after[u], case.ref[u]) for u in range(case.n))


# ------------------------------------------------------------------------------------------------- 6. errors
def test_errors_name_the_id_and_leave_no_trace(case):
    import q3t
    eng = case.eng
    V = eng.cfg["codec_vocab"]
    good = case.item(0, max_len=NF)

    def too_many(run, next_id, room, running, idle):
        return [good] * (room + 1), False

    with pytest.raises(q3t.Q3TError, match="utterance 0: the arrival callback returned 5 utterances for a room of 4"):
        Run(eng, 4, too_many, **case.kw)
    cases = [
        (dict(top_k=-1), {}, "top_k must be >= 0"),
        (dict(max_len=NF + 1), {}, "max_len exceeds the call's max_len"),
        (dict(language_id=V), {}, "language id out of range"),
        (dict(max_len=60), dict(max_len=60), "max_len exceeds the context reserved at ctx creation"),
    ]
    for bad, call_kw, msg in cases:
        kw = dict(case.kw, **call_kw)
        seen = []

        def script(run, next_id, room, running, idle):
            if next_id == 0:
                return [good], False
            return [dict(good, **bad)], False   # the second arrival, while the first runs

        with pytest.raises(q3t.Q3TError, match=f"utterance 1: {msg}"):
            r = Run(eng, 4, script, **kw)
            seen.append(r)
        assert not seen
        per = {k: v for k, v in dict(good, **bad).items() if k not in ("prompt", "speaker")}
        assert eng.check_utt(good["prompt"], good["speaker"], per_utt=per, **kw) == f"utterance 0: {msg}"
    per = {k: v for k, v in good.items() if k not in ("prompt", "speaker")}
    assert eng.check_utt(good["prompt"], good["speaker"], per_utt=per, **case.kw) is None
    assert "Need at least 4 text tokens" in eng.check_utt(good["prompt"][:3], per_utt=per, **case.kw)
    # the C entry point refuses a null callback and a bad interval
    lib = q3t.lib()
    p = q3t.default_params(**case.kw)
    cb = q3t.QUEUE_CB(lambda *a: 1)
    acb = q3t.ARRIVE_CB(lambda *a: 0)
    na, nf = C.c_int32(0), C.c_int32(0)
    for a, c, interval in ((acb, cb, 0), (acb, cb, -2), (q3t.ARRIVE_CB(), cb, 4), (acb, q3t.QUEUE_CB(), 4)):
        rc = lib.q3t_generate_queue_open(eng.h, C.byref(p), 0, 0, a, c, None, interval, C.byref(na), C.byref(nf))
        assert rc != 0 and lib.q3t_last_error().decode().strip(), interval
    # the next valid calls are unchanged
    run = Run(eng, 4, in_order([case.item(u) for u in range(case.n)], 3, (1, 2)), **case.kw)
    assert all(np.array_equal(run.cat(u), case.ref[u]) for u in range(case.n))
