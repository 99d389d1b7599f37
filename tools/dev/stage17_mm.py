"""dev: the 1.7B layout's batched stages on the matrix-core stack against the vector kernels (Q3T_MM17=0), the sibling
of stage17.py (its one-slot persistent frame).

Per slot count (default 16 and 64) and per pair, two child processes, one per setting of Q3T_MM17, alternating: each
loads full17 (tools/q3t_synth.c), reports q3t_decode_family and times the talker step and the code-predictor frame at
position 266 with q3t_time_stage.  The 64-slot children also run generate_queue of 256 utterances (natural EOS, max_len
48) through their 64 slots, warmed up by a 64-utterance queue, timed with the host clock.

    python tools/dev/stage17_mm.py [--pairs 3] [--slots 16 64] [--out profiles/mm17_stage.json]

Prints every child's line and a summary table (median, min..max over the pairs); --out keeps the raw lines as JSON."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
POS, N_UTT, MAX_LEN = 266, 256, 48


def child(slots, queue):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
    import numpy as np
    import q3t
    from q3t_testutil import prompt, synth_dir
    tts, _ = synth_dir("full17")
    eng = q3t.Engine(tts, None, max_slots=slots, max_ctx=330)
    r = dict(slots=slots, mm17=os.environ.get("Q3T_MM17", "1"), family=eng.decode_family(slots),
             talker_ms=eng.time_stage(0, slots, POS, 20), cp_frame_ms=eng.time_stage(1, slots, POS, 20))
    if queue:
        base = prompt("full17")
        rng = np.random.default_rng(11)
        prompts = [base[:4] + [int(t) for t in rng.integers(20, 920, int(rng.integers(10, 121)) - 4)] for _ in range(N_UTT)]
        spk = [np.zeros(eng.cfg["hidden"], np.float32)] * N_UTT
        kw = dict(max_len=MAX_LEN, temperature=0.9, top_k=50, seed=2024)
        eng.generate_queue(prompts[:slots], speakers=spk[:slots], **kw)
        t = time.perf_counter()
        out = eng.generate_queue(prompts, speakers=spk, **kw)
        r["queue_s"] = time.perf_counter() - t
        r["queue_frames"] = int(sum(len(c) for c in out))
    eng.close()
    print("RESULT " + json.dumps(r), flush=True)


def run_child(slots, mm17, queue):
    env = dict(os.environ, Q3T_MM17=mm17)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(slots)] + (["--queue"] if queue else [])
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout
    line = [l for l in out.splitlines() if l.startswith("RESULT ")][-1]
    print(line, flush=True)
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--queue", action="store_true")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--slots", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.queue)
    rows = []
    for slots in a.slots:
        for pair in range(a.pairs):
            for mm17 in (("1", "0") if pair % 2 == 0 else ("0", "1")):
                rows.append(dict(run_child(slots, mm17, slots == 64), pair=pair))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    print(f"{'slots':>5} {'Q3T_MM17':>8} {'family':>6} {'talker step ms':>26} {'code-predictor frame ms':>26} {'queue frames/s':>26}")
    for slots in a.slots:
        for mm17 in ("1", "0"):
            sel = [r for r in rows if r["slots"] == slots and r["mm17"] == mm17]

            def col(vals):
                return f"{statistics.median(vals):9.3f} ({min(vals):.3f}..{max(vals):.3f})" if vals else ""
            fps = [r["queue_frames"] / r["queue_s"] for r in sel if "queue_s" in r]
            print(f"{slots:>5} {mm17:>8} {sel[0]['family']:>6} {col([r['talker_ms'] for r in sel]):>26} "
                  f"{col([r['cp_frame_ms'] for r in sel]):>26} {col(fps):>26}")


if __name__ == "__main__":
    main()
