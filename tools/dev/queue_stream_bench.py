"""dev: the continuous-batching queue with deliveries (q3t_generate_queue_stream) and batched vocoder-stream pushes
sharing the GPU, end to end, on the full synthetic model.

Workload: 512 utterances with natural EOS (prompts of 10..120 tokens, max_len 512) through 64 slots, interval 12.
Lines, each timed with the host clock around the synchronous call, every shape warmed up (a 96-utterance queue of the
same slot count), --rounds alternating rounds, median and spread reported:
  1  generate_queue                                               frames/s
  2  generate_queue_stream, empty callback, no code buffers       frames/s
  2c the same with the code buffers kept (want_codes=True)        frames/s: line 1 plus the deliveries and nothing else
  3  generate_queue_stream, one batched push per callback         frames/s; per utterance the time from call start to
     (a pool of 64 vocoder streams, reset on reuse)               its first and final PCM (median, p95); time in the callback
  4  with --parent-root DIR (a built checkout of the parent commit), in a child process that imports THAT checkout's
     q3t: the same utterances in lock-step waves of 64 through generate_stream, the deliveries of an interval pushed as
     one batch (what Qwen3TTS::synthesize_batch does).  The reference line: frames/s and the same two latencies; an
     utterance's final PCM cannot come before its wave ends.
Writes one JSON document (--out) and prints a summary."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N_UTT, SLOTS, MAX_LEN, INTERVAL, N_WARM = 512, 64, 512, 12, 96
KW = dict(max_len=MAX_LEN, temperature=0.9, top_k=50, seed=2024)


def setup(root):
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, os.path.join(root, "qwen3-tts-jetson_amd"))
    import q3t
    from q3t_testutil import prompt, synth_dir
    tts, tok = synth_dir("full")
    eng = q3t.Engine(tts, tok, device=0, max_slots=SLOTS, max_ctx=MAX_LEN + 40)
    base = prompt("full")
    rng = np.random.default_rng(11)
    prompts = []
    for i in range(N_UTT):
        k = int(rng.integers(10, 121))
        body = [int(t) for t in rng.integers(20, 920, k - 4)]
        prompts.append(base[:4] + body)
    spk = [np.zeros(eng.cfg["hidden"], np.float32)] * N_UTT
    return q3t, eng, prompts, spk


def pct(v, q):
    return float(np.percentile(np.asarray(v, np.float64), q))


def lat(first, final):
    return dict(first_pcm_ms=dict(median=pct(first, 50), p95=pct(first, 95)),
                final_pcm_ms=dict(median=pct(final, 50), p95=pct(final, 95)))


def line1(eng, prompts, spk):
    t = time.perf_counter()
    out = eng.generate_queue(prompts, speakers=spk, **KW)
    dt = time.perf_counter() - t
    return dict(frames=int(sum(len(c) for c in out)), s=dt)


def line2(eng, prompts, spk, want_codes=False):
    t = time.perf_counter()
    out = eng.generate_queue_stream(prompts, lambda e: None, interval=INTERVAL, speakers=spk, want_codes=want_codes, **KW)
    dt = time.perf_counter() - t
    return dict(frames=int(sum(len(c) for c in out) if want_codes else sum(out)), s=dt)


def line3(eng, prompts, spk, pool):
    n = len(prompts)
    free, mine = list(pool), {}
    first, final = [None] * n, [None] * n
    in_cb = [0.0]
    t0 = time.perf_counter()

    def on_batch(entries):
        t = time.perf_counter()
        push = []
        for u, c, fin in entries:
            if u not in mine:
                mine[u] = free.pop()
                mine[u].reset()
            if len(c):
                push.append((u, c))
        if push:
            eng.vocoder_stream_push_batch([mine[u] for u, _ in push], [c for _, c in push])
        now = time.perf_counter()
        for u, _ in push:
            if first[u] is None:
                first[u] = (now - t0) * 1e3
        for u, _, fin in entries:
            if fin:
                final[u] = (now - t0) * 1e3
                free.append(mine.pop(u))
        in_cb[0] += now - t

    nf = eng.generate_queue_stream(prompts, on_batch, interval=INTERVAL, speakers=spk, want_codes=False, **KW)
    dt = time.perf_counter() - t0
    ok = [u for u in range(n) if first[u] is not None]
    return dict(frames=int(sum(nf)), s=dt, callback_s=in_cb[0], **lat([first[u] for u in ok], [final[u] for u in ok]))


def line4(eng, prompts, spk):
    """lock-step waves of SLOTS through generate_stream, one batched push per interval"""
    n = len(prompts)
    first, final = [None] * n, [None] * n
    frames, in_cb = 0, [0.0]
    t0 = time.perf_counter()
    for w in range(0, n, SLOTS):
        idx = list(range(w, min(n, w + SLOTS)))
        streams = [eng.vocoder_stream(max_frames=MAX_LEN) for _ in idx]
        pend = []

        def flush():
            if not pend:
                return
            t = time.perf_counter()
            eng.vocoder_stream_push_batch([streams[j] for j, _ in pend], [c for _, c in pend])
            now = time.perf_counter()
            for j, _ in pend:
                if first[idx[j]] is None:
                    first[idx[j]] = (now - t0) * 1e3
                final[idx[j]] = (now - t0) * 1e3
            in_cb[0] += now - t
            pend.clear()

        def on_frames(j, c):
            if pend and j <= pend[-1][0]:
                flush()
            if len(c):
                pend.append((j, c))
            return True

        out = eng.generate_stream([prompts[u] for u in idx], on_frames, interval=INTERVAL, speakers=[spk[u] for u in idx], **KW)
        flush()
        frames += sum(len(c) for c in out)
        for st in streams:
            st.close()
    dt = time.perf_counter() - t0
    ok = [u for u in range(n) if first[u] is not None]
    return dict(frames=int(frames), s=dt, callback_s=in_cb[0], **lat([first[u] for u in ok], [final[u] for u in ok]))


def child_parent(args):
    q3t, eng, prompts, spk = setup(args.parent_root)
    line4(eng, prompts[:N_WARM], spk[:N_WARM])
    for _ in range(args.rounds):
        print("LINE4 " + json.dumps(line4(eng, prompts, spk)), flush=True)
    eng.close()


def summarise(runs):
    fps = [r["frames"] / r["s"] for r in runs]
    m = statistics.median(fps)
    out = dict(frames=runs[0]["frames"], frames_per_s=m, spread=(min(fps) / m - 1, max(fps) / m - 1), runs=runs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit, for line 4")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "queue_stream_bench.json"))
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child == "parent":
        return child_parent(args)
    q3t, eng, prompts, spk = setup(REPO)
    pool = [eng.vocoder_stream(max_frames=MAX_LEN) for _ in range(SLOTS)]
    wp, ws = prompts[:N_WARM], spk[:N_WARM]
    line1(eng, wp, ws), line2(eng, wp, ws), line2(eng, wp, ws, True), line3(eng, wp, ws, pool)
    runs = {1: [], 2: [], "2c": [], 3: [], 4: []}
    for rnd in range(args.rounds):   # the parent's child runs after each of this build's rounds: the two alternate
        print(f"round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        runs[1].append(line1(eng, prompts, spk))
        runs[2].append(line2(eng, prompts, spk))
        runs["2c"].append(line2(eng, prompts, spk, True))
        runs[3].append(line3(eng, prompts, spk, pool))
        if args.parent_root:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "parent", "--rounds", "1",
                                "--parent-root", os.path.abspath(args.parent_root)], capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[4] += [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("LINE4 ")]
    eng.close()
    res = dict(workload=dict(n_utt=N_UTT, slots=SLOTS, interval=INTERVAL, rounds=args.rounds, **KW),
               generate_queue=summarise(runs[1]), queue_stream_empty_callback=summarise(runs[2]),
               queue_stream_empty_callback_with_codes=summarise(runs["2c"]),
               queue_stream_batched_push=summarise(runs[3]))
    if runs[4]:
        res["parent_lockstep_waves_batched_push"] = summarise(runs[4])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for k, v in res.items():
        if k == "workload":
            continue
        last = v["runs"][-1]
        extra = ""
        if "first_pcm_ms" in last:
            med = lambda key, q: statistics.median(r[key][q] for r in v["runs"])
            extra = (f"  first PCM {med('first_pcm_ms', 'median'):.0f} / {med('first_pcm_ms', 'p95'):.0f} ms, final PCM "
                     f"{med('final_pcm_ms', 'median'):.0f} / {med('final_pcm_ms', 'p95'):.0f} ms (median / p95), callback "
                     f"{statistics.median(r['callback_s'] / r['s'] for r in v['runs']) * 100:.0f}% of the wall time")
        print(f"{k:>38}: {v['frames_per_s']:9.0f} frames/s ({v['spread'][0] * 100:+.1f}/{v['spread'][1] * 100:+.1f}%), "
              f"{v['frames']} frames{extra}")


if __name__ == "__main__":
    main()
