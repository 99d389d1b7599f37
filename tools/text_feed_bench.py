"""What text feeds cost in the queue (DESIGN 2f "Text feeds"): 256 utterances of 40 text ids through 64 slots, 128
frames each (EOS masked), four ways --
  parent_queue   generate_queue of another build of the package (--parent-pkg DIR: a checkout of the parent commit,
                 built; left out without it)
  queue          generate_queue of this tree
  text_ahead     generate_queue_text, every utterance open with a head of one text id, everything fed at the first ask
  text_per_ask   generate_queue_text at interval 12, one id per ask: an utterance is asked at every tick and whenever
                 it has no row for its next frame, so after the head is used up there is a feed round between every
                 two frames (the most rounds a run can have)
-- as frames/s (wall clock around the call, which ends in a device synchronise) and, for the two text ways, the feed
rounds and their device time (an event pair around each round).  Each measurement runs in a process of its own,
parent and this tree alternating, --pairs times; every process warms up once (graph captures) and checks that the three
ways of this tree give the same codes.  The driver compares the parent's codes with this tree's by digest.

    python tools/text_feed_bench.py [--parent-pkg DIR] [--pairs 3] [--out profiles/text_feed_bench.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    sys.path.insert(0, args.pkg)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import q3t
    from q3t_testutil import prompt, synth_dir
    tts, _ = synth_dir("full")
    eng = q3t.Engine(tts, None, device=0, max_slots=args.slots, max_ctx=args.frames + 40)
    base = prompt("full")
    rng = np.random.default_rng(1)
    texts = [[int(x) for x in rng.integers(20, 920, args.ids)] for _ in range(args.utts)]
    whole = [base[:4] + t + base[-5:] for t in texts]
    heads = [base[:4] + t[:1] for t in texts]
    kw = dict(max_len=args.frames, force_frames=args.frames, temperature=0.9, top_k=50, repetition_penalty=1.05, seed=7)

    def digest(codes):
        return hashlib.sha1(b"".join(np.ascontiguousarray(c).tobytes() for c in codes)).hexdigest()

    def ahead():
        return eng.generate_queue_text(heads, [1] * args.utts, lambda u, f, a: (texts[u][1:], True), interval=12, **kw)[0]

    def per_ask():
        rest = [list(t[1:]) for t in texts]

        def src(u, f, a):
            r = rest[u]
            return [r.pop(0)], not r
        return eng.generate_queue_text(heads, [1] * args.utts, src, interval=12, **kw)[0]

    ways = {"queue": lambda: eng.generate_queue(whole, **kw)}
    if args.text:
        ways["text_ahead"] = ahead
        ways["text_per_ask"] = per_ask
    res = {}
    ref = None
    for name, fn in ways.items():
        fn()   # warm-up: graph captures, scratch
        t0 = time.perf_counter()
        codes = fn()
        dt = time.perf_counter() - t0
        frames = int(sum(len(c) for c in codes))
        res[name] = {"s": dt, "frames": frames, "frames_per_s": frames / dt, "digest": digest(codes)}
        if name != "queue":
            st = eng.text_feed_stats()
            res[name].update(st)
            res[name]["ms_per_feed_round"] = st["feed_ms"] / max(st["feed_rounds"], 1)
        ref = ref or res[name]["digest"]
        assert res[name]["digest"] == ref, f"{name}: codes differ from generate_queue's"
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--ids", type=int, default=40)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(REPO, "qwen3-tts-jetson_amd"))
    ap.add_argument("--text", type=int, default=1)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def run(pkg, text):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg", pkg, "--text", str(text)]
        for k in ("utts", "slots", "ids", "frames"):
            cmd += [f"--{k}", str(getattr(args, k))]
        out = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])

    runs = {}
    for _ in range(args.pairs):   # alternating, so a drift of the machine hits both
        if args.parent_pkg:
            runs.setdefault("parent_queue", []).append(run(args.parent_pkg, 0)["queue"])
        for name, r in run(args.pkg, 1).items():
            runs.setdefault(name, []).append(r)
    out = {"workload": {k: getattr(args, k) for k in ("utts", "slots", "ids", "frames", "pairs")}}
    for name, rs in runs.items():
        fps = sorted(r["frames_per_s"] for r in rs)
        med = fps[len(fps) // 2]
        out[name] = {"frames_per_s": med, "spread": [fps[0] / med - 1, fps[-1] / med - 1], "runs": rs}
    if "parent_queue" in runs:
        out["parent_codes_equal"] = all(a["digest"] == b["digest"] for a, b in zip(runs["parent_queue"], runs["queue"]))
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: (v if not isinstance(v, dict) or "runs" not in v else
                          {"frames_per_s": v["frames_per_s"], "spread": v["spread"]}) for k, v in out.items()}))


if __name__ == "__main__":
    main()
