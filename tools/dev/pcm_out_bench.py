"""dev: what the output stage adds to a batched vocoder-stream push, on the full synthetic model.

64 streams, each holding 266 frames, take 4 new frames in ONE call:
  plain   q3t_vocoder_stream_push_batch: f32 at 24 kHz copied back (this build, and with --parent-lib the parent
          commit's libq3t.so, which has no output stage)
  out     q3t_vocoder_stream_push_batch_out with an (8000, MULAW) spec on every stream: one conversion launch more,
          u8 at 8 kHz copied back (12x fewer bytes)
Host clock around the synchronous call (H2D codes, launches, D2H, stream synchronise: what a caller waits for).  Every
measurement is a child process of its own (one context, one warm-up call, --repeats timed calls; the streams are
re-opened and brought to their position before every timed call, untimed).  The children alternate: plain on this
build, plain on the parent, out on this build, --pairs times over, so drift of the machine falls on all three alike.
The launch count of the stage is read from q3t_pcm_out_launches around each `out` call.
Writes one JSON document (--out) and prints a table."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
THIS_LIB = os.path.join(REPO, "qwen3-tts-jetson_amd", "q3t", "libq3t.so")
S, POS, N = 64, 266, 4
RATE, MULAW = 8000, 2


class Spec(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("format", C.c_int32)]


def child(args):
    from q3t_testutil import synth_dir
    lib = C.CDLL(args.lib)
    lib.q3t_last_error.restype = C.c_char_p
    lib.q3t_vocoder_num_samples.restype = C.c_int64
    lib.q3t_vocoder_num_samples.argtypes = [C.c_void_p, C.c_int32, C.c_int]
    lib.q3t_vocoder_stream_open.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.q3t_vocoder_stream_push_batch.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    lib.q3t_vocoder_stream_close.restype = None
    lib.q3t_vocoder_stream_close.argtypes = [C.c_void_p]
    lib.q3t_ctx_destroy.argtypes = [C.c_void_p]
    out = args.child == "out"
    if out:
        lib.q3t_pcm_num_samples.restype = C.c_int64
        lib.q3t_pcm_num_samples.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        lib.q3t_vocoder_stream_set_output.argtypes = [C.c_void_p, C.c_void_p]
        lib.q3t_vocoder_stream_push_batch_out.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        lib.q3t_pcm_out_launches.restype = C.c_int64
    ctx = C.c_void_p()
    _, tok = synth_dir("full")
    assert lib.q3t_ctx_create(None, tok.encode(), 0, 1, 32, C.byref(ctx)) == 0, lib.q3t_last_error()
    codes = np.random.default_rng(0).integers(0, 2048, (POS + N + S, 16)).astype(np.int32)
    nsamp = lambda F: lib.q3t_vocoder_num_samples(ctx, F, 0)
    spec = Spec(RATE, MULAW)
    ns = (C.c_int64 * S)()
    arr = lambda ct, v: (ct * S)(*v)
    times, launches, nbytes = [], [], 0
    for it in range(args.repeats + 1):          # the first call is the warm-up
        hs = []
        for _ in range(S):
            h = C.c_void_p()
            assert lib.q3t_vocoder_stream_open(ctx, POS + N, C.byref(h)) == 0, lib.q3t_last_error()
            if out:
                assert lib.q3t_vocoder_stream_set_output(h, C.byref(spec)) == 0, lib.q3t_last_error()
            hs.append(h)
        harr = arr(C.c_void_p, [h.value for h in hs])
        pre = [np.ascontiguousarray(codes[j:j + POS]) for j in range(S)]
        new = [np.ascontiguousarray(codes[j + POS:j + POS + N]) for j in range(S)]
        if out:
            cap0 = lib.q3t_pcm_num_samples(nsamp(POS), RATE, 0)
            cap1 = lib.q3t_pcm_num_samples(nsamp(POS + N), RATE, 0) - cap0
            b0 = [np.zeros(cap0, np.uint8) for _ in range(S)]
            b1 = [np.zeros(cap1, np.uint8) for _ in range(S)]
            assert lib.q3t_vocoder_stream_push_batch_out(harr, S, arr(C.c_void_p, [x.ctypes.data for x in pre]),
                                                         arr(C.c_int32, [POS] * S), None, arr(C.c_void_p, [b.ctypes.data for b in b0]),
                                                         arr(C.c_int64, [cap0] * S), ns) == 0, lib.q3t_last_error()
            a = (harr, S, arr(C.c_void_p, [x.ctypes.data for x in new]), arr(C.c_int32, [N] * S), None,
                 arr(C.c_void_p, [b.ctypes.data for b in b1]), arr(C.c_int64, [cap1] * S), ns)
            before = lib.q3t_pcm_out_launches()
            t = time.perf_counter()
            rc = lib.q3t_vocoder_stream_push_batch_out(*a)
            dt = (time.perf_counter() - t) * 1e3
            launches.append(lib.q3t_pcm_out_launches() - before)
            nbytes = cap1 * S
        else:
            cap0, cap1 = nsamp(POS), nsamp(POS + N) - nsamp(POS)
            b0 = [np.zeros(cap0, np.float32) for _ in range(S)]
            b1 = [np.zeros(cap1, np.float32) for _ in range(S)]
            assert lib.q3t_vocoder_stream_push_batch(harr, S, arr(C.c_void_p, [x.ctypes.data for x in pre]),
                                                     arr(C.c_int32, [POS] * S), arr(C.c_void_p, [b.ctypes.data for b in b0]),
                                                     arr(C.c_int64, [cap0] * S), ns) == 0, lib.q3t_last_error()
            a = (harr, S, arr(C.c_void_p, [x.ctypes.data for x in new]), arr(C.c_int32, [N] * S),
                 arr(C.c_void_p, [b.ctypes.data for b in b1]), arr(C.c_int64, [cap1] * S), ns)
            t = time.perf_counter()
            rc = lib.q3t_vocoder_stream_push_batch(*a)
            dt = (time.perf_counter() - t) * 1e3
            nbytes = cap1 * S * 4
        assert rc == 0, lib.q3t_last_error()
        if it:
            times.append(dt)
        for h in hs:
            lib.q3t_vocoder_stream_close(h)
    lib.q3t_ctx_destroy(ctx)
    print("RESULT " + json.dumps(dict(ms=times, launches=launches[1:], bytes_back=nbytes)), flush=True)


def run_child(kind, lib, repeats):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--lib", lib, "--repeats", str(repeats)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="path of the parent commit's libq3t.so")
    ap.add_argument("--lib", default=THIS_LIB)
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "bench_out_pcm_out", "pcm_out_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    runs = []
    for p in range(args.pairs):
        row = dict(pair=p, plain=run_child("plain", THIS_LIB, args.repeats))
        if args.parent_lib:
            row["parent"] = run_child("plain", os.path.abspath(args.parent_lib), args.repeats)
        row["out"] = run_child("out", THIS_LIB, args.repeats)
        runs.append(row)
        print(f"pair {p}: " + "  ".join(f"{k} {statistics.median(v['ms']):.3f} ms (min {min(v['ms']):.3f}, max {max(v['ms']):.3f})"
                                         for k, v in row.items() if k != "pair"), flush=True)
    launches = sorted({n for r in runs for n in r["out"]["launches"]})
    res = dict(streams=S, position=POS, frames=N, spec=[RATE, MULAW], repeats=args.repeats, runs=runs,
               conversion_launches_per_out_call=launches,
               bytes_back=dict(plain=runs[0]["plain"]["bytes_back"], out=runs[0]["out"]["bytes_back"]))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"conversion launches per _out call: {launches}; bytes copied back per call: plain {res['bytes_back']['plain']}, "
          f"out {res['bytes_back']['out']}")


if __name__ == "__main__":
    main()
