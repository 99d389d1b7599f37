"""Queue deliveries (q3t_generate_queue_stream): the continuous-batching queue hands frames out while it runs.

The `full` synthetic model and the prompts of test_gpu_queue.py, so that both EOS stops and max_len stops occur (both
asserted).  Checked per utterance, against q3t_generate_queue on the same context:

  equality     the concatenated deliveries are generate_queue's codes, bit for bit and in length, with all, 3 and 1
               utterance in flight and an interval (5) that does not divide max_len (48)
  contract     deliveries in order; a non-final one has 1..interval frames; exactly one final one, of 0..interval
               frames, and nothing after it; a delivery that is not the first and leaves the utterance unfinished (fewer
               frames handed out so far than the utterance has) has exactly `interval` frames
  early        an utterance's final delivery comes when it ends, not when the call does
  cancel       an utterance stopped at its first delivery gets nothing more and keeps that length; the others are
               unchanged
  late cancel  an utterance stopped at its last piece before the final one -- which may be handed out after the
               utterance ended and left its slot -- is as long as what it was handed, with and without code buffers
  abort        returning False ends the call with n_frames = what was handed out
  one slot     the same equality on the persistent one-slot kernels
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu
NF, INTERVAL = 48, 5
KW = dict(max_len=NF, temperature=0.9, top_k=50, seed=123)


def _prompts(n, seed):   # test_gpu_queue.py::_prompts
    base = prompt("full")
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(5, 13))
        tail = [(t + 13 * i) % 900 + 20 for t in base[4:]]
        out.append(base[:4] + tail[:k - 4])
    return out


class Case:
    def __init__(self, slots, n_utt):
        import q3t
        tts, _ = synth_dir("full")
        self.slots, self.n_utt = slots, n_utt
        self.eng = q3t.Engine(tts, None, device=0, max_slots=slots, max_ctx=NF + 40)
        self.prompts = _prompts(n_utt, slots)
        self.spk = [np.zeros(self.eng.cfg["hidden"], np.float32)] * n_utt
        self.ref = self.eng.generate_queue(self.prompts, speakers=self.spk, **KW)   # computed once, never changed

    def stream(self, on_batch=None, **kw):
        """-> (return value, log of (utt, codes, final) in delivery order with the callback's ordinal)"""
        log = []
        calls = [0]

        def cb(entries):
            assert [e[0] for e in entries] == sorted(e[0] for e in entries) and len(entries) > 0
            for u, c, fin in entries:
                log.append((u, c, fin, calls[0]))
            calls[0] += 1
            return on_batch(entries) if on_batch else None
        out = self.eng.generate_queue_stream(self.prompts, cb, interval=INTERVAL, speakers=self.spk, **dict(KW, **kw))
        return out, log


@pytest.fixture(scope="module", params=[(4, 10), (12, 20)], ids=["4x10", "12x20"])
def case(request):
    c = Case(*request.param)
    yield c
    c.eng.close()


def check_contract(log, lengths, n_utt, skip=()):
    """the per-utterance contract; lengths[u]: the utterance's frame count.  Returns the concatenations"""
    per = {u: [] for u in range(n_utt)}
    for u, c, fin, _ in log:
        per[u].append((c, fin))
    cat = {}
    for u in range(n_utt):
        if u in skip:
            continue
        d = per[u]
        assert d and [fin for _, fin in d].count(True) == 1 and d[-1][1], (u, [(len(c), fin) for c, fin in d])
        got = 0
        for i, (c, fin) in enumerate(d):
            n = len(c)
            assert (0 if fin else 1) <= n <= INTERVAL, (u, i, n, fin)
            got += n
            if i > 0 and got < lengths[u]:
                assert n == INTERVAL, (u, i, n, got, lengths[u])
        cat[u] = np.concatenate([c for c, _ in d]) if d else np.zeros((0, 16), np.int32)
    return cat


@pytest.mark.parametrize("active", ["all", 3, 1])
def test_deliveries_equal_generate_queue(case, active):
    lens = [len(c) for c in case.ref]
    assert any(n < NF for n in lens) and any(n == NF for n in lens), f"need EOS stops and max_len stops: {lens}"
    out, log = case.stream(max_active=case.slots if active == "all" else active)
    cat = check_contract(log, lens, case.n_utt)
    for u in range(case.n_utt):
        assert np.array_equal(out[u], case.ref[u]), (u, len(out[u]), lens[u])
        assert np.array_equal(cat[u], case.ref[u]), (u, len(cat[u]), lens[u])


def test_an_utterance_is_reported_when_it_ends(case):
    _, log = case.stream()
    finals = 0
    first = {}
    first_final = None
    for i, (u, c, fin, _) in enumerate(log):
        if u not in first:
            first[u] = i
            if u >= case.slots:   # it took the slot of an utterance that ended: those were reported before
                assert finals >= u - case.slots + 1, (u, finals)
        if fin:
            finals += 1
            if first_final is None:
                first_final = i
    assert first_final < first[case.n_utt - 1]


def test_without_code_buffers_the_deliveries_are_the_same(case):
    lens = [len(c) for c in case.ref]
    nf, log = case.stream(want_codes=False)
    assert nf == lens
    cat = check_contract(log, lens, case.n_utt)
    for u in range(case.n_utt):
        assert np.array_equal(cat[u], case.ref[u]), u


def test_cancel_one_utterance(case):
    seen = []

    def stop_one(entries):
        hit = [u for u, _, _ in entries if u == 1 and not seen]
        seen.extend(hit)
        return hit
    out, log = case.stream(stop_one)
    mine = [(c, fin) for u, c, fin, _ in log if u == 1]
    assert len(mine) == 1 and not mine[0][1] and 1 <= len(mine[0][0]) < len(case.ref[1])
    assert np.array_equal(out[1], mine[0][0]) and np.array_equal(out[1], case.ref[1][:len(out[1])])
    cat = check_contract(log, [len(c) for c in case.ref], case.n_utt, skip=(1,))
    for u in range(case.n_utt):
        if u != 1:
            assert np.array_equal(out[u], case.ref[u]) and np.array_equal(cat[u], case.ref[u]), u


@pytest.mark.parametrize("want_codes", [True, False], ids=["codes", "no-codes"])
def test_cancel_at_the_last_piece_before_the_final(case, want_codes):
    """the piece after which 1..interval frames are left: by the time it is handed out (a tick late) the utterance
    has often ended and its slot been released; its length must still be what the callback was handed"""
    lens = [len(c) for c in case.ref]
    handed = {u: 0 for u in range(case.n_utt)}
    stopped = set()

    def stop_late(entries):
        hit = []
        for u, c, fin in entries:
            assert u not in stopped, f"utterance {u} was delivered to after its cancel"
            handed[u] += len(c)
            if not fin and lens[u] - INTERVAL <= handed[u] < lens[u]:
                hit.append(u)
                stopped.add(u)
        return hit
    out, _ = case.stream(stop_late, want_codes=want_codes)
    assert len(stopped) >= case.n_utt // 2, (sorted(stopped), lens)
    for u in range(case.n_utt):
        assert (handed[u] < lens[u]) == (u in stopped), (u, handed[u], lens[u])
        if want_codes:
            assert len(out[u]) == handed[u] and np.array_equal(out[u], case.ref[u][:handed[u]]), (u, len(out[u]), handed[u])
        else:
            assert out[u] == handed[u], (u, out[u], handed[u], lens[u])


def test_abort(case):
    calls = []

    def abort_at_third(entries):
        calls.append(1)
        return len(calls) < 3
    out, log = case.stream(abort_at_third)
    assert len(calls) == 3
    handed = {u: 0 for u in range(case.n_utt)}
    for u, c, _, _ in log:
        handed[u] += len(c)
    assert sum(handed.values()) > 0
    for u in range(case.n_utt):
        assert len(out[u]) == handed[u] and np.array_equal(out[u], case.ref[u][:handed[u]]), u
    again, _ = case.stream()   # the context is as usable as before
    assert all(np.array_equal(a, b) for a, b in zip(again, case.ref))


def test_one_slot_runs_the_persistent_kernels():
    import q3t
    tts, _ = synth_dir("full")
    eng = q3t.Engine(tts, None, device=0, max_slots=1, max_ctx=NF + 40)
    try:
        prompts = _prompts(3, 4)
        spk = [np.zeros(eng.cfg["hidden"], np.float32)] * 3
        ref = eng.generate_queue(prompts, speakers=spk, **KW)
        log = []
        out = eng.generate_queue_stream(prompts, lambda e: log.extend((u, c, f, 0) for u, c, f in e), interval=INTERVAL,
                                        speakers=spk, **KW)
        cat = check_contract(log, [len(c) for c in ref], 3)
        for u in range(3):
            assert np.array_equal(out[u], ref[u]) and np.array_equal(cat[u], ref[u]), u
        assert eng.persist_status() == 0 and eng.persist_kernels() != 0, (eng.persist_status(), eng.persist_kernels())
    finally:
        eng.close()


def test_errors(case):
    import q3t
    lib = q3t.lib()
    n = 2
    toks = [np.ascontiguousarray(t, np.int32) for t in case.prompts[:n]]
    tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
    ntok = np.array([len(t) for t in toks], np.int32)
    p = q3t.default_params(**KW)
    nf = np.zeros(n, np.int32)
    cb = q3t.QUEUE_CB(lambda *a: 1)
    null_cb = q3t.QUEUE_CB()
    for bad_cb, interval in ((cb, 0), (cb, -3), (null_cb, INTERVAL)):
        rc = lib.q3t_generate_queue_stream(case.eng.h, n, tarr, ntok, None, C.byref(p), None, nf, 0, bad_cb, None, interval)
        assert rc != 0 and lib.q3t_last_error().decode().strip(), (interval, rc)
