"""The open queue's host side without a GPU.

  scheduler     tests/cpp/test_queue_arrivals.cpp, built with g++ against qwen3-tts-jetson_amd/csrc/queue_sched.h (which must
                compile without HIP): when the arrival callback is asked and with which room and idle, never with a batch in
                flight or after the close, the loop's end at close plus drain, abort, a queue that goes empty and takes up
                work again, the arrival log's replay after a scripted fault, 100,000 arrivals through 4 slots with bounded
                tables, and every rejection's message
  ArrivalQueue  q3t.ArrivalQueue driven by threads and a consumer that plays the engine: order, ids, and that the source
                blocks only when it is told the engine is idle.  No clock: the consumer's steps are sequenced by events
  ABI           the new entry points are exported and refuse null callbacks without a context's device
"""
import ctypes as C
import os
import subprocess
import sys
import threading

from q3t_testutil import REPO

PKG = os.path.join(REPO, "qwen3-tts-jetson_amd")


def test_queue_arrivals(tmp_path):
    exe = str(tmp_path / "test_queue_arrivals")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tests", "cpp", "test_queue_arrivals.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def _q3t():
    sys.path.insert(0, PKG)
    import q3t
    return q3t


def test_arrival_queue_order_and_ids():
    q3t = _q3t()
    aq = q3t.ArrivalQueue()
    ids = [aq.submit([1, 2, 3, 4, i], temperature=0.5 + i) for i in range(5)]
    assert ids == [0, 1, 2, 3, 4]
    assert aq.submit([9], key=77, speaker="s") == 5
    # not idle: what is there and fits, at once, in submission order
    got, closed = aq.source(0, 2, 3, False)
    assert [g["prompt"][-1] for g in got] == [0, 1] and not closed
    assert [g["key"] for g in got] == [0, 1] and got[1]["temperature"] == 1.5 and got[0]["speaker"] is None
    got, closed = aq.source(2, 8, 1, False)
    assert [g["key"] for g in got] == [2, 3, 4, 77] and got[3]["speaker"] == "s" and not closed
    # empty and not idle: returns at once with nothing
    assert aq.source(6, 4, 1, False) == ([], False)
    aq.close()
    assert aq.source(6, 4, 0, True) == ([], True)     # closed and drained: idle does not block either
    try:
        aq.submit([1])
    except ValueError:
        pass
    else:
        raise AssertionError("submit after close must fail")
    # a close with requests left: they are handed over first, closed comes with the last of them
    b = q3t.ArrivalQueue()
    for i in range(3):
        b.submit([i])
    b.close()
    got, closed = b.source(0, 2, 0, True)
    assert len(got) == 2 and not closed
    got, closed = b.source(2, 2, 1, False)
    assert len(got) == 1 and closed


def test_arrival_queue_blocks_only_when_idle():
    """A consumer thread plays the engine.  With idle false and nothing queued it must come back by itself (the main thread
    submits nothing until it has); with idle true it must stay inside source() until a producer thread submits."""
    q3t = _q3t()
    aq = q3t.ArrivalQueue()
    back = threading.Event()
    entered = threading.Event()
    result = {}

    def consumer():
        result["busy"] = aq.source(0, 4, 2, False)   # nothing there, not idle: returns at once
        back.set()
        entered.set()
        result["idle"] = aq.source(0, 4, 0, True)    # idle: waits for the producer
        result["after"] = aq.source(1, 4, 1, False)

    t = threading.Thread(target=consumer)
    t.start()
    assert back.wait(30), "source() blocked although the engine was not idle"
    assert result["busy"] == ([], False)
    assert entered.wait(30)
    assert "idle" not in result    # nobody has submitted: the idle ask cannot have returned
    ids = []
    producers = [threading.Thread(target=lambda i=i: ids.append(aq.submit([i]))) for i in range(1)]
    for p in producers:
        p.start()
    for p in producers:
        p.join()
    t.join(30)
    assert not t.is_alive()
    got, closed = result["idle"]
    assert len(got) == 1 and got[0]["key"] == 0 and not closed and ids == [0]
    assert result["after"] == ([], False)
    # many producers: every id handed out once, the ids the source hands over are in submission (id) order
    many = q3t.ArrivalQueue()
    seen = []
    lock = threading.Lock()

    def produce(n):
        for _ in range(n):
            i = many.submit([0])
            with lock:
                seen.append(i)

    ts = [threading.Thread(target=produce, args=(50,)) for _ in range(4)]
    for x in ts:
        x.start()
    for x in ts:
        x.join()
    many.close()
    assert sorted(seen) == list(range(200))
    keys = []
    closed = False
    while not closed:
        got, closed = many.source(len(keys), 7, 0, True)
        keys += [g["key"] for g in got]
    assert keys == list(range(200))


def test_open_queue_abi_without_device():
    q3t = _q3t()
    lib = C.CDLL(q3t.LIB_PATH)
    assert "q3t_generate_queue_open" in q3t.EXPORTS and "q3t_check_utt" in q3t.EXPORTS
    lib.q3t_last_error.restype = C.c_char_p
    na, nf = C.c_int32(5), C.c_int32(5)
    rc = lib.q3t_generate_queue_open(None, None, 0, 0, None, None, None, 12, C.byref(na), C.byref(nf))
    assert rc != 0 and lib.q3t_last_error().decode().strip() and na.value == 0 and nf.value == 0
    assert lib.q3t_check_utt(None, None, 0, None, None, None) != 0
    hdr = open(os.path.join(REPO, "include", "q3t_backend.h")).read()
    assert "also while an idle ask blocks" in hdr   # the lock rule is stated where callers read it
