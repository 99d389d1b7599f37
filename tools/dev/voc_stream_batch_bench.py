"""dev: what a batched vocoder-stream push (q3t_vocoder_stream_push_batch) costs against the same pushes made one
after the other, on the full synthetic model.

For S in 1, 4, 16, 64 streams and n in 4, 12 new frames per stream, every stream holding 266 frames, and for one mixed
row (64 streams, 12 frames, positions spread over 40..512) it times, with the host clock around the synchronous calls
(H2D codes, launches, D2H PCM, stream synchronise: what a caller waits for), every shape warmed up, medians of
--repeats runs in --rounds rounds:
  (a) ONE q3t_vocoder_stream_push_batch over the S streams (this build);
  (b) S q3t_vocoder_stream_push calls in a row (this build);
  (c) with --parent-lib PATH: S q3t_vocoder_stream_push calls in a row on another build of libq3t.so (the parent
      commit's) in a child process, its rounds interleaved with the rounds of (a) and (b).  The baseline of the
      reported ratio is (c), never this build.
Streams are opened and brought to their position again before every timed call (not timed), so every run measures the
same positions.  All three go through the same ctypes calls on preallocated buffers.
--profile runs one `rocprofv3 --kernel-trace --stats` of its own (no counters) over a child that makes three 64-stream
pushes of 12 frames from position 266, cuts the trace at k_codes_cols (the first launch of every push) and reports the
launches per batched call against 64 x the launches of a single push measured the same way.
Writes one JSON document (--out) and prints a table."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
THIS_LIB = os.path.join(REPO, "qwen3-tts-jetson_amd", "q3t", "libq3t.so")

POS = 266
SHAPES = [(S, n, "266") for n in (4, 12) for S in (1, 4, 16, 64)] + [(64, 12, "40..512")]


def positions(S, kind):
    return [POS] * S if kind == "266" else [int(p) for p in np.linspace(40, 512, S)]


def key(S, n, kind):
    return f"S={S} n={n} P={kind}"


class Raw:
    """the stream calls of one build of libq3t.so through ctypes alone (the parent's build has no batched push for the
    q3t module to bind)"""

    def __init__(self, lib_path):
        from q3t_testutil import synth_dir
        lib = self.lib = C.CDLL(lib_path)
        lib.q3t_last_error.restype = C.c_char_p
        lib.q3t_vocoder_num_samples.restype = C.c_int64
        lib.q3t_vocoder_num_samples.argtypes = [C.c_void_p, C.c_int32, C.c_int]
        lib.q3t_vocoder_stream_open.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        lib.q3t_vocoder_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        lib.q3t_vocoder_stream_close.restype = None
        lib.q3t_vocoder_stream_close.argtypes = [C.c_void_p]
        lib.q3t_ctx_destroy.argtypes = [C.c_void_p]
        self.has_batch = hasattr(lib, "q3t_vocoder_stream_push_batch")
        if self.has_batch:
            lib.q3t_vocoder_stream_push_batch.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
            lib.q3t_vocoder_stream_last_groups.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        _, tok = synth_dir("full")
        rc = lib.q3t_ctx_create(None, tok.encode(), 0, 1, 32, C.byref(self.h))
        assert rc == 0, lib.q3t_last_error()

    def nsamp(self, F):
        return self.lib.q3t_vocoder_num_samples(self.h, F, 0)

    def close(self):
        self.lib.q3t_ctx_destroy(self.h)


class Round:
    """S streams at their positions, the arguments of the next push of n frames ready"""

    def __init__(self, raw, c, Ps, n):
        self.raw, self.S = raw, len(Ps)
        S = self.S
        self.h = []
        for P in Ps:
            h = C.c_void_p()
            assert raw.lib.q3t_vocoder_stream_open(raw.h, P + n, C.byref(h)) == 0, raw.lib.q3t_last_error()
            self.h.append(h)
        self.ns = (C.c_int64 * S)()
        # bring every stream to its position (batched where the build can: it is not what is timed)
        pre = [np.ascontiguousarray(c[j:j + P]) for j, P in enumerate(Ps)]
        self.push(pre, [raw.nsamp(P) for P in Ps], batched=raw.has_batch)
        self.codes = [np.ascontiguousarray(c[j + P:j + P + n]) for j, P in enumerate(Ps)]
        self.caps = [raw.nsamp(P + n) - raw.nsamp(P) for P in Ps]
        self.pcm = [np.zeros(k, np.float32) for k in self.caps]
        self.args = ((C.c_void_p * S)(*[h.value for h in self.h]), (C.c_void_p * S)(*[x.ctypes.data for x in self.codes]),
                     (C.c_int32 * S)(*[n] * S), (C.c_void_p * S)(*[p.ctypes.data for p in self.pcm]),
                     (C.c_int64 * S)(*self.caps))
        self.n = n

    def push(self, codes, caps, batched):
        lib, S = self.raw.lib, self.S
        pcm = [np.zeros(max(k, 1), np.float32) for k in caps]
        if batched:
            rc = lib.q3t_vocoder_stream_push_batch((C.c_void_p * S)(*[h.value for h in self.h]), S,
                                                   (C.c_void_p * S)(*[x.ctypes.data for x in codes]),
                                                   (C.c_int32 * S)(*[x.shape[0] for x in codes]),
                                                   (C.c_void_p * S)(*[p.ctypes.data for p in pcm]), (C.c_int64 * S)(*caps), self.ns)
            assert rc == 0, lib.q3t_last_error()
        else:
            for h, x, p, k in zip(self.h, codes, pcm, caps):
                assert lib.q3t_vocoder_stream_push(h, x.ctypes.data, x.shape[0], p.ctypes.data, k, self.ns) == 0, lib.q3t_last_error()

    def timed(self, batched):
        lib, S, n = self.raw.lib, self.S, self.n
        hs, cs, nf, ps, caps = self.args
        t = time.perf_counter()
        if batched:
            rc = lib.q3t_vocoder_stream_push_batch(hs, S, cs, nf, ps, caps, self.ns)
        else:
            rc = 0
            for j in range(S):
                rc |= lib.q3t_vocoder_stream_push(hs[j], cs[j], n, ps[j], caps[j], self.ns)
        dt = (time.perf_counter() - t) * 1e3
        assert rc == 0, lib.q3t_last_error()
        return dt

    def close(self):
        for h in self.h:
            self.raw.lib.q3t_vocoder_stream_close(h)


def codes():
    return np.random.default_rng(0).integers(0, 2048, (512 + 12 + 64, 16)).astype(np.int32)


def one(raw, c, S, n, kind, batched):
    r = Round(raw, c, positions(S, kind), n)
    try:
        dt = r.timed(batched)
        groups = raw.lib.q3t_vocoder_stream_last_groups(raw.h) if batched else None
    finally:
        r.close()
    return dt, groups


def child_serial(args):
    raw = Raw(args.lib)
    c = codes()
    for S, n, kind in SHAPES:   # warm-up of every shape
        one(raw, c, S, n, kind, False)
    out = {key(*sh): [one(raw, c, *sh, False)[0] for _ in range(args.repeats)] for sh in SHAPES}
    print("SERIAL " + json.dumps(out), flush=True)
    raw.close()


def child_profile(args):
    raw = Raw(THIS_LIB)
    c = codes()
    one(raw, c, 64, 12, "266", True)   # warm-up
    one(raw, c, 1, 12, "266", False)
    print("MARK single", flush=True)
    one(raw, c, 1, 12, "266", False)
    for _ in range(3):
        one(raw, c, 64, 12, "266", True)
    raw.close()


def profile(outdir):
    d = os.path.join(outdir, "voc_stream_batch_prof")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "push", "--",
           sys.executable, os.path.abspath(__file__), "--child", "profile"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"error": r.stderr[-2000:]}
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not trace:
        return {"error": "no kernel_trace.csv under " + d}
    if stats:
        shutil.copy(stats[0], os.path.join(outdir, "voc_stream_batch_push_kernel_stats.csv"))
    rows = []
    with open(trace[0]) as f:
        for x in csv.DictReader(f):
            rows.append((int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]))
    rows.sort()
    cuts = [i for i, x in enumerate(rows) if "k_codes_cols" in x[2]]
    calls = [rows[a:b] for a, b in zip(cuts, cuts[1:] + [len(rows)])]
    # the child's last seven calls: prefill + push of one single stream, then three times (batched prefill, batched push)
    single, batched = calls[-7], [calls[-5], calls[-3], calls[-1]]
    def summary(p):
        return dict(launches=len(p), busy_us=sum(e - s for s, e, _ in p) / 1e3, span_us=(p[-1][1] - p[0][0]) / 1e3)
    b = [summary(p) for p in batched]
    return dict(single_push=summary(single), batched_push_64=b[-1], batched_launches=[x["launches"] for x in b],
                serial_64_launches=64 * len(single),
                batch_kernels=sorted({nm.split("(")[0][-60:] for _, _, nm in batched[-1] if "batch" in nm}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="rounds the repeats are split into (parent rounds in between)")
    ap.add_argument("--parent-lib", default="", help="path of the parent commit's libq3t.so for (c)")
    ap.add_argument("--lib", default="", help="(child) the library --child serial loads")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "bench_out_voc_stream", "voc_stream_batch_bench.json"))
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child == "serial":
        return child_serial(args)
    if args.child == "profile":
        return child_profile(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    raw = Raw(THIS_LIB)
    c = codes()
    a = {key(*sh): [] for sh in SHAPES}
    b = {k: [] for k in a}
    bp = {k: [] for k in a}
    groups = {}
    for sh in SHAPES:   # warm-up of every shape
        one(raw, c, *sh, True)
        one(raw, c, *sh, False)
    per = max(1, args.repeats // args.rounds)
    for rnd in range(args.rounds):
        print(f"round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        for _ in range(per):
            for sh in SHAPES:
                dt, g = one(raw, c, *sh, True)
                a[key(*sh)].append(dt)
                groups[key(*sh)] = g
                b[key(*sh)].append(one(raw, c, *sh, False)[0])
        if args.parent_lib:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "serial", "--repeats", str(per),
                                "--lib", os.path.abspath(args.parent_lib)], capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SERIAL ")][-1][7:])
            for k, v in got.items():
                bp[k] += v
    raw.close()
    med = statistics.median
    rows = {}
    for S, n, kind in SHAPES:
        k = key(S, n, kind)
        m = med(a[k])
        row = dict(streams=S, n=n, positions=kind, groups=groups[k], batch_ms=m, batch_ms_per_stream=m / S,
                   batch_spread=(min(a[k]) / m - 1, max(a[k]) / m - 1),
                   serial_ms=med(b[k]), serial_ms_per_stream=med(b[k]) / S)
        if bp[k]:
            pm = med(bp[k])
            row.update(parent_serial_ms=pm, parent_serial_ms_per_stream=pm / S, batch_over_parent=m / pm,
                       parent_spread=(min(bp[k]) / pm - 1, max(bp[k]) / pm - 1))
        rows[k] = row
    res = dict(repeats=per * args.rounds, rows=rows)
    if args.profile:
        res["profile"] = profile(os.path.dirname(args.out))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"{'shape':>22} {'groups':>6} {'batch ms':>9} {'/stream':>8} {'spread':>13} {'serial ms':>10} {'parent ms':>10} {'/stream':>8} {'batch/parent':>12}")
    for k, r in rows.items():
        sp = f"{r['batch_spread'][0] * 100:+.0f}/{r['batch_spread'][1] * 100:+.0f}%"
        p, pp, ratio = r.get("parent_serial_ms"), r.get("parent_serial_ms_per_stream"), r.get("batch_over_parent")
        f3 = lambda v: "-" if v is None else f"{v:.3f}"
        print(f"{k:>22} {r['groups']:>6} {r['batch_ms']:9.3f} {r['batch_ms_per_stream']:8.3f} {sp:>13} {r['serial_ms']:10.3f} "
              f"{f3(p):>10} {f3(pp):>8} {f3(ratio):>12}")
    if args.profile:
        print("profile:", json.dumps(res["profile"], indent=1))


if __name__ == "__main__":
    main()
