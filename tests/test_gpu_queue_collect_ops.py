"""The queue's collection kernel alone (k_queue_collect), through the test-only shim
tests/queue_ops/libq3t_queue_ops.so, against a numpy restatement of its contract (csrc/kernels.h, QueueCollect); the
comparison is exact.

Shapes: S = 5 slots, interval = 4, codes_max_len = 9, max_len = 7.  Staging rows, header and the guard rows around the
chunk are pre-filled with a poison value.  One slot each: n = 0; n = interval; EOS with done < frame (rows at and after
done must not be copied); avail clipped by max_len with frame > max_len; a slot left out of the mask (rows, header and
counter untouched).  A second launch over the same state gives n = 0 everywhere.  A counter far behind (n > interval)
sets the error word and writes nothing outside (or inside) the chunk's rows.
"""
import numpy as np
import pytest

import queue_ops_lib

pytestmark = pytest.mark.gpu

S, INTERVAL, CML, MAX_LEN = 5, 4, 9, 7
POISON = np.int32(-0x5A5A5A5B)
G = 3   # guard slots' worth of rows in front of and behind the staging chunk


@pytest.fixture(scope="module")
def ops():
    return queue_ops_lib.load()


def restate(mask, done, frame, delivered, codes, rows, header):
    """the contract, slot by slot; returns the error word"""
    err = 0
    for k in range(S):
        if not mask[k]:
            continue
        avail = min(done[k], MAX_LEN) if done[k] >= 0 else min(frame[k], MAX_LEN)
        n = avail - delivered[k]
        if delivered[k] < 0 or n < 0 or n > INTERVAL:
            err = 1
            header[k] = 0
            continue
        rows[k, :n] = codes[k, delivered[k]:avail]
        header[k] = n
        delivered[k] = avail
    return err


class State:
    def __init__(self, ops, mask, done, frame, delivered):
        rng = np.random.default_rng(7)
        self.ops = ops
        self.mask = np.asarray(mask, np.int32)
        self.done = np.asarray(done, np.int32)
        self.frame = np.asarray(frame, np.int32)
        self.delivered = np.asarray(delivered, np.int32)
        self.codes = rng.integers(0, 2048, (S, CML, 16)).astype(np.int32)
        self.rows = np.full((S + 2 * G, INTERVAL, 16), POISON, np.int32)   # the chunk is rows[G : G + S]
        self.header = np.full(S + 2, POISON, np.int32)                    # the header is header[1 : 1 + S]
        self.error = np.zeros(1, np.int32)
        D = ops.DevBuf
        self.d = {n: D(getattr(self, n)) for n in ("mask", "done", "frame", "delivered", "codes", "rows", "header", "error")}

    def launch(self):
        d = self.d
        self.ops.call("collect", d["mask"].p, d["done"].p, d["frame"].p, d["delivered"].p, d["codes"].p,
                      d["rows"].p + G * INTERVAL * 64, d["header"].p + 4, d["error"].p, S, INTERVAL, CML, MAX_LEN)
        self.error[0] |= restate(self.mask, self.done, self.frame, self.delivered, self.codes,
                                 self.rows[G:G + S], self.header[1:1 + S])

    def check(self):
        for n in ("delivered", "rows", "header", "error", "codes", "done", "frame", "mask"):
            want = getattr(self, n)
            got = self.d[n].get(np.int32, want.size).reshape(want.shape)
            assert np.array_equal(got, want), f"{n} differs:\n{got}\nwant\n{want}"


def test_collect_cases_and_second_launch(ops):
    #            n = 0   n = interval   EOS, done < frame   frame > max_len   not in the mask
    st = State(ops, mask=[1, 1, 1, 1, 0], done=[-1, -1, 5, -1, -1], frame=[3, 6, 8, 9, 6], delivered=[3, 2, 3, 4, 1])
    st.launch()
    assert list(st.header[1:1 + S]) == [0, INTERVAL, 2, 3, POISON]   # the restatement covers the cases named above
    assert list(st.delivered) == [3, 6, 5, 7, 1] and st.error[0] == 0
    assert (st.rows[G + 2, 2:] == POISON).all() and (st.rows[G + 4] == POISON).all()
    st.check()
    st.launch()   # nothing new: n = 0 for every selected slot, rows unchanged
    assert list(st.header[1:1 + S]) == [0, 0, 0, 0, POISON]
    st.check()


def test_counter_far_behind_sets_the_error_word(ops):
    # slot 1 and slot 4 (the chunk's last) are 6 and 7 frames behind: n > interval; slot 2 has a negative counter
    st = State(ops, mask=[1, 1, 1, 0, 1], done=[-1, -1, -1, -1, 7], frame=[2, 6, 3, 1, 7], delivered=[1, 0, -2, 0, 0])
    st.launch()
    assert st.error[0] == 1
    assert list(st.header[1:1 + S]) == [1, 0, 0, POISON, 0] and list(st.delivered) == [2, 0, -2, 0, 0]
    assert (st.rows[:G] == POISON).all() and (st.rows[G + 1:] == POISON).all()   # only slot 0's first row was written
    st.check()
