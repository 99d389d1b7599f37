"""What per-utterance records cost in the queue: 256 utterances through 64 slots three ways --
  old      q3t_generate_queue (one q3t_gen_params for all)
  same     q3t_generate_queue_utt with identical records (what `old` computes, through the record / ragged paths)
  mixed    q3t_generate_queue_utt with the language / speaker mix of tests/test_gpu_utt_params.py (prompts of 8, 9 and 10
           rows in one admission batch)
-- frames/s of each (wall clock around the call, best and median of --reps), and the admission prefill on its own:
64 prompts through q3t_talker_prefill (uniform, 9 rows each) and q3t_talker_prefill_ragged (the same rows, and a mix of
8 / 9 / 10 rows), wall clock per call including its upload and its synchronisation.  Prints one JSON line.

    python tools/dev/utt_queue_bench.py [--utts 256] [--slots 64] [--frames 64] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import q3t
    from q3t_testutil import prompt, synth_dir
    tts, _ = synth_dir("full")
    eng = q3t.Engine(tts, None, device=0, max_slots=args.slots, max_ctx=args.frames + 40)
    H = eng.cfg["hidden"]
    base = prompt("full")
    rng = np.random.default_rng(1)
    prompts = []
    for i in range(args.utts):
        k = int(rng.integers(5, 13))
        prompts.append(base[:4] + [(t + 13 * i) % 900 + 20 for t in base[4:]][:k - 4])
    spk = [(rng.standard_normal(H) * 0.02).astype(np.float32) for _ in range(args.utts)]
    kw = dict(max_len=args.frames, temperature=0.9, top_k=50, repetition_penalty=1.05, seed=7)
    classes = [(2050, True), (2050, False), (-1, True), (2055, False), (-1, False)]
    mix_spk = [spk[u] if classes[u % 5][1] else None for u in range(args.utts)]
    mix_up = [dict(language_id=classes[u % 5][0]) for u in range(args.utts)]
    ways = {
        "old": lambda: eng.generate_queue(prompts, speakers=spk, **kw),
        "same": lambda: eng.generate_queue(prompts, speakers=spk, per_utt=[None] * args.utts, **kw),
        "mixed": lambda: eng.generate_queue(prompts, speakers=mix_spk, per_utt=mix_up, **kw),
    }
    res = {"utts": args.utts, "slots": args.slots, "max_len": args.frames, "reps": args.reps}
    outs = {}
    for name, fn in ways.items():
        outs[name] = fn()   # warm-up: graph captures
    times = {name: [] for name in ways}
    for _ in range(args.reps):   # interleaved, so a drift of the box hits all three
        for name, fn in ways.items():
            eng.synchronize()
            t = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t)
    for name in ways:
        frames = sum(len(c) for c in outs[name])
        res[name] = {"frames": frames, "best_s": round(min(times[name]), 4), "median_s": round(statistics.median(times[name]), 4),
                     "frames_per_s_best": round(frames / min(times[name]), 1),
                     "frames_per_s_median": round(frames / statistics.median(times[name]), 1)}
    res["same_equals_old"] = all(np.array_equal(a, b) for a, b in zip(outs["old"], outs["same"]))
    # ---- the admission batch's prefill alone, in the 64-slot family
    n = args.slots
    rows9 = (rng.standard_normal((n, 9, H)) * 0.5).astype(np.float32)
    lens = [(10, 9, 9, 9, 8)[u % 5] for u in range(n)]
    ragged = [(rng.standard_normal((k, H)) * 0.5).astype(np.float32) for k in lens]

    def timed(fn, iters=30):
        fn()
        ts = []
        for _ in range(iters):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return round(statistics.median(ts), 4)

    res["prefill_ms"] = {
        "rows": {"uniform9": 9 * n, "mixed": int(sum(lens))},
        "uniform": timed(lambda: eng.talker_prefill(rows9, family_slots=n)),
        "ragged_same_rows": timed(lambda: eng.talker_prefill_ragged(list(rows9), family_slots=n)),
        "ragged_mixed": timed(lambda: eng.talker_prefill_ragged(ragged, family_slots=n)),
    }
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
