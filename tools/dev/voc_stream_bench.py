"""dev: what a vocoder-stream push costs, on the full synthetic model.

At stream positions 40, 266 and 512 frames it times (host clock around calls that end in a stream synchronise and
return the PCM: the latency a caller sees; medians of --repeats runs after a warm-up of every shape)
  (a) a push of 4, 12 and 40 frames into a stream holding `pos` frames;
  (b) the exact alternative without a stream: a one-shot FULL decode of all pos + n frames -- on this build, and with
      --parent-lib PATH on another build of libq3t.so (e.g. the parent commit's) in a child process, its rounds
      interleaved with the rounds of (a);
  (c) q3t_vocoder_decode_chunked of one 40-frame chunk, the inexact streaming path.
--profile runs one `rocprofv3 --kernel-trace --stats` of its own over a child that pushes 12 frames ten times from position
266, cuts the trace into pushes at k_codes_cols (the first launch of every push) and reports, per push, the launch
count, the kernels' busy time against the span from the first launch's start to the last one's end, and the shares of
the two stream kernels and of the convolution stack (every launch after output_proj's, the last GEMV); the halo's part
of the stack is estimated by rows, halo / (halo + n).
Writes one JSON document (--out) and prints a table."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

POSITIONS = (40, 266, 512)
PIECES = (4, 12, 40)


def engine():
    import q3t
    from q3t_testutil import synth_dir
    _, tok = synth_dir("full")
    return q3t.Engine(None, tok, device=0)


def codes(F):
    return np.random.default_rng(0).integers(0, 2048, (F, 16)).astype(np.int32)


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def push_ms(eng, c, pos, n):
    """one push of n frames into a stream holding pos frames (the prefill push is not timed)"""
    with eng.vocoder_stream(max_frames=pos + n) as st:
        st.push(c[:pos])
        return timed(lambda: st.push(c[pos:pos + n]))


def oneshot_round(eng, c, repeats):
    return {f"{pos}+{n}": [timed(lambda: eng.vocoder(c[:pos + n], 0)) for _ in range(repeats)]
            for pos in POSITIONS for n in PIECES}


class RawEngine:
    """q3t_vocoder_decode of another build of the library through ctypes alone (a build from before the stream has
    no q3t_vocoder_stream_* for the q3t module to bind)"""

    def __init__(self, lib_path):
        import ctypes as C
        from q3t_testutil import synth_dir
        self.C, self.lib = C, C.CDLL(lib_path)
        self.lib.q3t_last_error.restype = C.c_char_p
        self.lib.q3t_vocoder_num_samples.restype = C.c_int64
        self.lib.q3t_vocoder_num_samples.argtypes = [C.c_void_p, C.c_int32, C.c_int]
        self.lib.q3t_vocoder_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p]
        self.lib.q3t_ctx_destroy.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        _, tok = synth_dir("full")
        rc = self.lib.q3t_ctx_create(None, tok.encode(), 0, 1, 32, C.byref(self.h))
        assert rc == 0, self.lib.q3t_last_error()

    def vocoder(self, c, mode):
        C = self.C
        c = np.ascontiguousarray(c, np.int32)
        pcm = np.zeros(self.lib.q3t_vocoder_num_samples(self.h, c.shape[0], mode), np.float32)
        ns = C.c_int64(0)
        rc = self.lib.q3t_vocoder_decode(self.h, c.ctypes.data_as(C.c_void_p), c.shape[0], mode,
                                         pcm.ctypes.data_as(C.c_void_p), C.byref(ns))
        assert rc == 0, self.lib.q3t_last_error()
        return pcm[:ns.value]

    def close(self):
        self.lib.q3t_ctx_destroy(self.h)


def child_oneshot(args):
    eng = RawEngine(args.lib)
    c = codes(max(POSITIONS) + max(PIECES))
    oneshot_round(eng, c, 1)   # warm-up of every shape
    print("ONESHOT " + json.dumps(oneshot_round(eng, c, args.repeats)), flush=True)
    eng.close()


def child_profile(args):
    eng = engine()
    c = codes(266 + 12 * 12)
    with eng.vocoder_stream(max_frames=c.shape[0]) as st:
        st.push(c[:254])
        st.push(c[254:266])   # warm-up of the push shape
        for i in range(10):
            st.push(c[266 + 12 * i:266 + 12 * (i + 1)])
        print(f"HALO {st.halo}", flush=True)
    eng.close()


def profile(args, outdir):
    d = os.path.join(outdir, "voc_stream_prof")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "push", "--",
           sys.executable, os.path.abspath(__file__), "--child", "profile"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return {"error": r.stderr[-2000:]}
    halo = int([ln for ln in r.stdout.splitlines() if ln.startswith("HALO ")][-1].split()[1])
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        return {"error": "no kernel_trace.csv under " + d}
    rows = []
    with open(trace[0]) as f:
        for x in csv.DictReader(f):
            rows.append((int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]))
    rows.sort()
    cuts = [i for i, x in enumerate(rows) if "k_codes_cols" in x[2]]
    pushes = [rows[a:b] for a, b in zip(cuts, cuts[1:] + [len(rows)])][-10:]   # the ten timed pushes
    out = []
    for p in pushes:
        busy = sum(e - s for s, e, _ in p)
        span = p[-1][1] - p[0][0]
        last_gemv = max(i for i, x in enumerate(p) if "gemv" in x[2].lower() or "gemm" in x[2].lower())
        stack = sum(e - s for s, e, _ in p[last_gemv + 1:])
        attn = sum(e - s for s, e, nm in p if "k_voc_attn_cached" in nm)
        app = sum(e - s for s, e, nm in p if "k_voc_kv_append" in nm)
        out.append(dict(launches=len(p), busy_us=busy / 1e3, span_us=span / 1e3, stack_us=stack / 1e3,
                        attn_cached_us=attn / 1e3, kv_append_us=app / 1e3))
    med = {k: statistics.median(x[k] for x in out) for k in out[0]}
    n = 12
    med.update(halo=halo, n=n, pos="266..374",
               share_attn_cached=med["attn_cached_us"] / med["busy_us"], share_kv_append=med["kv_append_us"] / med["busy_us"],
               share_stack=med["stack_us"] / med["busy_us"],
               share_halo_recompute_est=med["stack_us"] / med["busy_us"] * halo / (halo + n),
               busy_over_span=med["busy_us"] / med["span_us"],
               kernels=sorted({nm.split("(")[0][-60:] for _, _, nm in pushes[-1]}))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="rounds the repeats are split into (parent rounds in between)")
    ap.add_argument("--parent-lib", default="", help="path of another build of libq3t.so for (b), e.g. the parent commit's")
    ap.add_argument("--lib", default="", help="(child) the library --child oneshot loads")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "bench_out_voc_stream", "voc_stream_bench.json"))
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child == "oneshot":
        return child_oneshot(args)
    if args.child == "profile":
        return child_profile(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    eng = engine()
    c = codes(max(POSITIONS) + max(PIECES))
    a = {f"{pos}+{n}": [] for pos in POSITIONS for n in PIECES}
    b = {k: [] for k in a}
    bp = {k: [] for k in a}
    cc = []
    for pos in POSITIONS:   # warm-up of every shape
        for n in PIECES:
            push_ms(eng, c, pos, n)
    oneshot_round(eng, c, 1)
    eng.vocoder_chunked(c[:40], 40)
    per = max(1, args.repeats // args.rounds)
    for _ in range(args.rounds):
        for _ in range(per):
            for pos in POSITIONS:
                for n in PIECES:
                    a[f"{pos}+{n}"].append(push_ms(eng, c, pos, n))
                    b[f"{pos}+{n}"].append(timed(lambda: eng.vocoder(c[:pos + n], 0)))
            cc.append(timed(lambda: eng.vocoder_chunked(c[:40], 40)))
        if args.parent_lib:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "oneshot", "--repeats", str(per),
                                "--lib", os.path.abspath(args.parent_lib)], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ONESHOT ")][-1][8:])
            for k, v in got.items():
                bp[k] += v
    eng.close()
    med = statistics.median
    res = dict(repeats=per * args.rounds, push_ms={k: med(v) for k, v in a.items()},
               push_ms_min_max={k: (min(v), max(v)) for k, v in a.items()},
               oneshot_ms={k: med(v) for k, v in b.items()},
               oneshot_parent_ms={k: med(v) for k, v in bp.items() if v}, chunk40_ms=med(cc))
    if args.profile:
        res["profile"] = profile(args, os.path.dirname(args.out))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"{'pos+n':>8} {'push ms':>9} {'one-shot ms':>12} {'parent one-shot ms':>19}")
    for k in a:
        p = res["oneshot_parent_ms"].get(k)
        print(f"{k:>8} {res['push_ms'][k]:9.3f} {res['oneshot_ms'][k]:12.3f} {p if p is None else round(p, 3)!s:>19}")
    print(f"chunked, one 40-frame chunk: {res['chunk40_ms']:.3f} ms")
    if args.profile:
        print("profile:", json.dumps(res["profile"], indent=1))


if __name__ == "__main__":
    main()
