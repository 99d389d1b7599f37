"""The text-feed kernels alone (k_text_append, k_slot_hold), through the test-only shim
tests/text_ops/libq3t_text_ops.so, against numpy restatements of their contracts (csrc/kernels.h: TextAppend, SlotHold).
Every comparison is exact.

append        4 slots, max_trailing 8, H 1024 and H 64.  Rows for 3 of the 4 slots at different offsets; one slot
              closes (its last row is the shared tts_eos source row, trailing_len = K + 1), one slot gets no row and no
              commit.  The trailing buffer, trailing_len and n_tokens equal the restatement; every row no descriptor
              names keeps its poison value, as do the guard rows around the buffer.  A descriptor that names a row
              outside the buffers writes nothing and sets the error word.
hold/release  4 slots whose done is {-1, -1, 5, 0}, all in the mask but one of the running two: only a masked slot with
              done < 0 is held (hidden row saved, done = frame, flag set); the hidden rows are then overwritten, as a
              frame run on the held slot does, and the release restores the held slot's row bit for bit, sets done = -1
              and clears the flag.  A real EOS (done 5, done 0) is never cleared, by either launch.
"""
import numpy as np
import pytest

import text_ops_lib

pytestmark = pytest.mark.gpu

S, MT = 4, 8
POISON = np.float32(-7.25e11)
IPOISON = np.int32(-0x5A5A5A5B)


@pytest.fixture(scope="module")
def ops():
    return text_ops_lib.load()


def _append(ops, H, rows, commit, src_rows):
    """one launch; returns (trailing with one guard slot each side, trailing_len, n_tokens, error, src)"""
    rng = np.random.default_rng(H)
    src = rng.standard_normal((src_rows, H)).astype(np.float32)
    tr = np.full((S + 2, MT, H), POISON, np.float32)
    tl = np.full(S + 2, IPOISON, np.int32)
    nt = np.full(S + 2, IPOISON, np.int32)
    rows = np.asarray(rows, np.int32).reshape(-1, 3)
    commit = np.asarray(commit, np.int32).reshape(-1, 3)
    D = ops.DevBuf
    d_src, d_tr, d_tl, d_nt = D(src), D(tr), D(tl), D(nt)
    d_rows, d_commit, d_err = D(rows if rows.size else np.zeros(3, np.int32)), D(commit if commit.size else np.zeros(3, np.int32)), D(np.zeros(1, np.int32))
    ops.call("append", d_src.p, d_tr.p + MT * H * 4, d_rows.p, d_commit.p, d_tl.p + 4, d_nt.p + 4, d_err.p,
             len(rows), len(commit), src_rows, S, MT, H)
    return (d_tr.get(np.float32, tr.size).reshape(tr.shape), d_tl.get(np.int32, S + 2), d_nt.get(np.int32, S + 2),
            int(d_err.get(np.int32, 1)[0]), src)


@pytest.mark.parametrize("H", [1024, 64])
def test_append_rows_and_counters(ops, H):
    # slot 0: rows 2, 3 (K 2 -> 4); slot 1: nothing; slot 2: row 0, then closes (row 1 = the eos source row 5);
    # slot 3: rows 5, 6, 7 up to the end of its buffer (K 5 -> 8 = max_trailing, still open)
    rows = [(0, 0, 2), (1, 0, 3), (2, 2, 0), (5, 2, 1), (3, 3, 5), (4, 3, 6), (1, 3, 7)]
    commit = [(0, 4, 13), (2, 2, 10), (3, 8, 17)]
    tr, tl, nt, err, src = _append(ops, H, rows, commit, 6)
    want = np.full((S + 2, MT, H), POISON, np.float32)
    for s, k, d in rows:
        want[1 + k, d] = src[s]
    assert err == 0
    assert np.array_equal(tr, want)
    assert (tr[0] == POISON).all() and (tr[-1] == POISON).all() and (tr[2] == POISON).all()   # guards, the slot without a row
    assert list(tl) == [IPOISON, 4, IPOISON, 2, 8, IPOISON]
    assert list(nt) == [IPOISON, 13, IPOISON, 10, 17, IPOISON]


def test_append_descriptor_outside_the_buffers_is_skipped(ops):
    H = 64
    # a destination row at max_trailing, a slot at S, a source row at src_rows; a commit with trailing_len > max_trailing
    rows = [(0, 0, MT), (0, S, 0), (3, 1, 0), (1, 1, 1)]
    commit = [(1, MT + 1, 9), (2, 3, 12)]
    tr, tl, nt, err, src = _append(ops, H, rows, commit, 3)
    want = np.full((S + 2, MT, H), POISON, np.float32)
    want[1 + 1, 1] = src[1]
    assert err == 1
    assert np.array_equal(tr, want)
    assert list(tl) == [IPOISON, IPOISON, IPOISON, 3, IPOISON, IPOISON] and list(nt) == [IPOISON, IPOISON, IPOISON, 12, IPOISON, IPOISON]


@pytest.mark.parametrize("H", [1024, 64])
def test_hold_then_release(ops, H):
    rng = np.random.default_rng(3)
    hidden = rng.standard_normal((S, H)).astype(np.float32)
    done = np.array([-1, -1, 5, 0], np.int32)
    frame = np.array([7, 3, 4, 0], np.int32)
    mask = np.array([1, 0, 1, 1], np.int32)   # slot 1 runs on beside the held one
    D = ops.DevBuf
    d_mask, d_hid, d_done, d_frame = D(mask), D(hidden), D(done), D(frame)
    d_save, d_held = D(np.full((S, H), POISON, np.float32)), D(np.zeros(S, np.int32))
    ops.call("hold", d_mask.p, d_hid.p, d_save.p, d_done.p, d_held.p, d_frame.p, S, H, 0)
    assert list(d_done.get(np.int32, S)) == [7, -1, 5, 0]          # done = frame for the held slot; the EOS values stay
    assert list(d_held.get(np.int32, S)) == [1, 0, 0, 0]
    save = d_save.get(np.float32, S * H).reshape(S, H)
    assert np.array_equal(save[0], hidden[0]) and (save[1:] == POISON).all()
    assert np.array_equal(d_hid.get(np.float32, S * H).reshape(S, H), hidden)
    # frames run meanwhile: every slot's hidden row is overwritten
    later = rng.standard_normal((S, H)).astype(np.float32)
    d_hid2 = D(later)
    all_slots = D(np.ones(S, np.int32))
    ops.call("hold", all_slots.p, d_hid2.p, d_save.p, d_done.p, d_held.p, d_frame.p, S, H, 1)
    got = d_hid2.get(np.float32, S * H).reshape(S, H)
    assert np.array_equal(got[0], hidden[0])                       # restored bit for bit
    assert np.array_equal(got[1:], later[1:])                      # slots that were not held: untouched
    assert list(d_done.get(np.int32, S)) == [-1, -1, 5, 0]         # a real EOS is never cleared
    assert list(d_held.get(np.int32, S)) == [0, 0, 0, 0]
    # a second release finds nothing held
    ops.call("hold", all_slots.p, d_hid2.p, d_save.p, d_done.p, d_held.p, d_frame.p, S, H, 1)
    assert np.array_equal(d_hid2.get(np.float32, S * H).reshape(S, H), got)
    assert list(d_done.get(np.int32, S)) == [-1, -1, 5, 0]
