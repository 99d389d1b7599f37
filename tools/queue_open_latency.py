"""What the open queue buys and what its asks cost (DESIGN 2f "Arrivals"): 512 utterances with natural EOS (prompts of
5..12 ids, max_len 96) through 64 slots on the 0.6B synthetic weights.

  (a) wait   the utterances arrive on a fixed seeded schedule, about one per two frames (exponential gaps whose mean is
             twice the frame time measured in the warm-up).  Per utterance: the wall time from its arrival to its first
             delivery, median and 95th percentile, for
               open     Engine.generate_queue_open: an arrival is handed over at the first ask after it
               closed   the regime without it, emulated with generate_queue_stream: what has arrived forms a queue,
                        arrivals that come while it runs wait for it to drain and form the next queue
  (b) asks   total frames/s of the open call with every utterance handed over as soon as there is room, against
             generate_queue_stream (with records) on the same 512, three alternating repeats of each in one process; the
             codes of the two are compared.  The per-iteration ask is the only host work the open call adds.

    python tools/queue_open_latency.py [--out profiles/queue_open_latency.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--max-len", type=int, default=96)
    ap.add_argument("--interval", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "queue_open_latency.json"))
    args = ap.parse_args()
    import q3t
    from q3t_testutil import prompt, synth_dir
    tts, _ = synth_dir("full")
    eng = q3t.Engine(tts, None, device=0, max_slots=args.slots, max_ctx=args.max_len + 40)
    base = prompt("full")
    rng = np.random.default_rng(1)
    n = args.utts
    prompts = []
    for i in range(n):
        k = int(rng.integers(5, 13))
        prompts.append(base[:4] + [(t + 13 * i) % 900 + 20 for t in base[4:]][:k - 4])
    kw = dict(max_len=args.max_len, temperature=0.9, top_k=50, repetition_penalty=1.05, seed=7)
    recs = [None] * n

    def closed_all():
        return eng.generate_queue_stream(prompts, lambda e: None, interval=args.interval, per_utt=recs, **kw)

    def open_all():
        pieces = {}
        state = {"next": 0}

        def source(next_id, room, running, idle):
            a = state["next"]
            b = min(n, a + room)
            state["next"] = b
            return [dict(prompt=prompts[u]) for u in range(a, b)], b == n

        def on_batch(entries):
            for u, c, _ in entries:
                pieces.setdefault(u, []).append(c)
        eng.generate_queue_open(source, on_batch, interval=args.interval, slots=args.slots, **kw)
        return [np.concatenate(pieces[u]) if pieces.get(u) else np.zeros((0, 16), np.int32) for u in range(n)]

    # ---- (b) the cost of the asks (and the warm-up of both paths: graph captures, scratch)
    ref = closed_all()
    got = open_all()
    equal = all(np.array_equal(a, b) for a, b in zip(ref, got))
    frames = int(sum(len(c) for c in ref))
    lens = [len(c) for c in ref]
    runs = {"closed": [], "open": []}
    for _ in range(3):
        for name, fn in (("closed", closed_all), ("open", open_all)):
            t0 = time.perf_counter()
            fn()
            runs[name].append(frames / (time.perf_counter() - t0))
    # the frame time of a full queue, for the schedule: loop iterations ~ frames / slots
    frame_s = args.slots / float(np.median(runs["closed"]))

    # ---- (a) the wait from arrival to first delivery
    gaps = np.random.default_rng(2).exponential(2.0 * frame_s, n)
    arrive = np.cumsum(gaps)

    def wait_open():
        first = {}
        state = {"next": 0}
        t0 = time.perf_counter()

        def source(next_id, room, running, idle):
            a = state["next"]
            if idle and a < n:   # nothing runs: wait for the next arrival
                time.sleep(max(0.0, arrive[a] - (time.perf_counter() - t0)))
            now = time.perf_counter() - t0
            b = a
            while b < n and b - a < room and arrive[b] <= now:
                b += 1
            state["next"] = b
            return [dict(prompt=prompts[u]) for u in range(a, b)], b == n

        def on_batch(entries):
            now = time.perf_counter() - t0
            for u, c, _ in entries:
                first.setdefault(u, now)
        eng.generate_queue_open(source, on_batch, interval=args.interval, slots=args.slots, **kw)
        return np.array([first[u] - arrive[u] for u in range(n)])

    def wait_closed():
        first = {}
        t0 = time.perf_counter()
        a = 0
        while a < n:
            time.sleep(max(0.0, arrive[a] - (time.perf_counter() - t0)))
            now = time.perf_counter() - t0
            b = a
            while b < n and arrive[b] <= now:
                b += 1
            b = max(b, a + 1)

            def on_batch(entries, a=a):
                t = time.perf_counter() - t0
                for u, c, _ in entries:
                    first.setdefault(a + u, t)
            # (its utterances are keyed from 0 again: the emulation is about the waits, not the codes)
            eng.generate_queue_stream(prompts[a:b], on_batch, interval=args.interval, per_utt=recs[a:b], **kw)
            a = b
        return np.array([first[u] - arrive[u] for u in range(n)])

    w_open = wait_open()
    w_closed = wait_closed()

    def stats(w):
        return {"median_ms": float(np.median(w) * 1e3), "p95_ms": float(np.percentile(w, 95) * 1e3), "max_ms": float(w.max() * 1e3)}

    out = {
        "utts": n, "slots": args.slots, "max_len": args.max_len, "interval": args.interval,
        "frames": frames, "eos_stops": int(sum(x < args.max_len for x in lens)), "max_len_stops": int(sum(x == args.max_len for x in lens)),
        "asks": {"frames_per_s": runs, "open_over_closed": float(np.median(runs["open"]) / np.median(runs["closed"])),
                 "closed_spread": float((max(runs["closed"]) - min(runs["closed"])) / np.median(runs["closed"])),
                 "open_spread": float((max(runs["open"]) - min(runs["open"])) / np.median(runs["open"])),
                 "codes_equal": bool(equal)},
        "wait": {"frame_ms": frame_s * 1e3, "mean_gap_ms": float(gaps.mean() * 1e3), "open": stats(w_open), "closed": stats(w_closed)},
    }
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
