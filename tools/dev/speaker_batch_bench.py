"""dev: what the ragged batched speaker encoder saves, on the full synthetic model.

encode   Engine.encode_speakers of n three-second clips (n = 1, 4, 16) against n Engine.encode_speaker calls, on one
         context after a warm-up of both, alternating, --repeats times each.  Both calls return synchronised (upload,
         launches, copy back, stream synchronise: what a caller waits for); the time is taken with the host clock and
         with HIP events on the null stream around the call.  The encoder's launch counter is read around each.
arrival  one arrival round of the open queue with 4 new references while 4 slots decode: the source of
         Engine.generate_queue_open encodes the 4 clips inside the arrival callback, between two frames, batched or one
         by one (alternating runs).  The time of that encode is the stall it puts between two frames.
Writes one JSON document (--out) and prints a table."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
SR = 24000


def voice_like(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f0 = 140 + 30 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(np.sin(k * ph) / k for k in range(1, 12))
    x *= 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t) ** 2
    x += 0.02 * rng.standard_normal(len(t))
    return (0.3 * x / np.abs(x).max()).astype(np.float32)


class Events:
    """a pair of HIP events on the null stream around a synchronous call"""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time(self, fn):
        self.hip.hipEventRecord(self.a, None)
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        self.hip.hipEventRecord(self.b, None)
        self.hip.hipEventSynchronize(self.b)
        ms = C.c_float(0)
        self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b)
        return host, float(ms.value)


def med(v):
    return round(statistics.median(v), 3) if v else None


def bench_encode(q3t, eng, repeats):
    ev = Events()
    rows = []
    clips = [voice_like(3 * SR, seed=50 + i) for i in range(16)]
    launches = q3t.lib().q3t_speaker_launches
    for n in (1, 4, 16):
        sub = clips[:n]
        batch = lambda: eng.encode_speakers(sub)
        loop = lambda: [eng.encode_speaker(c) for c in sub]
        batch(), loop()   # warm-up (scratch sized, code objects loaded)
        l0 = launches(); batch(); lb = launches() - l0
        l0 = launches(); loop(); ll = launches() - l0
        tb, tl = [], []
        for _ in range(repeats):
            tb.append(ev.time(batch))
            tl.append(ev.time(loop))
        rows.append(dict(clips=n, batch_host_ms=med([t[0] for t in tb]), batch_event_ms=med([t[1] for t in tb]),
                         loop_host_ms=med([t[0] for t in tl]), loop_event_ms=med([t[1] for t in tl]),
                         batch_launches=lb, loop_launches=ll))
        print(f"encode  {n:2d} clips: batched {rows[-1]['batch_host_ms']:8.3f} ms host ({rows[-1]['batch_event_ms']:8.3f} events, "
              f"{lb} launches)   one by one {rows[-1]['loop_host_ms']:8.3f} ms host ({rows[-1]['loop_event_ms']:8.3f} events, "
              f"{ll} launches)")
    return rows


def bench_arrival(q3t, eng, runs):
    from q3t_testutil import prompt
    toks = prompt("full")
    clips = [voice_like(3 * SR, seed=80 + i) for i in range(4)]
    first = eng.encode_speakers(clips)[0]
    out = dict(batched=[], one_by_one=[])
    for run in range(2 * runs):
        mode = "batched" if run % 2 == 0 else "one_by_one"
        state = dict(round=0)

        def source(next_id, room, running, idle):
            if state["round"] == 0:
                state["round"] = 1
                return [dict(prompt=toks, speaker=first[i]) for i in range(4)], False
            if state["round"] == 1 and running == 4 and room >= 4:
                state["round"] = 2
                t0 = time.perf_counter()
                emb = eng.encode_speakers(clips)[0] if mode == "batched" else [eng.encode_speaker(c) for c in clips]
                out[mode].append((time.perf_counter() - t0) * 1e3)
                return [dict(prompt=toks, speaker=emb[i]) for i in range(4)], True
            return [], state["round"] == 2 or idle   # (never wait: nothing more comes once the slots are idle)

        eng.generate_queue_open(source, lambda entries: None, interval=4, slots=8, max_len=24, temperature=0.0, force_frames=24)
    res = {k: dict(median_ms=med(v), runs=[round(x, 3) for x in v]) for k, v in out.items()}
    for k, v in res.items():
        print(f"arrival 4 new references beside 4 decoding slots, {k:10s}: {v['median_ms']} ms between two frames")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--arrival-runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import q3t
    from q3t_testutil import synth_dir
    tts, tok = synth_dir("full")
    eng = q3t.Engine(tts, tok, device=0, max_slots=8, max_ctx=128)
    try:
        doc = dict(encode=bench_encode(q3t, eng, args.repeats), arrival=bench_arrival(q3t, eng, args.arrival_runs))
    finally:
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
