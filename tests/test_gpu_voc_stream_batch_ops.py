"""The batched vocoder-stream launchers alone (voc_kv_append_batch, voc_attn_cached_batch, voc_copy_batch), through
the test-only shim tests/voc_stream_batch_ops/libq3t_voc_stream_batch_ops.so, against the single-stream launchers
(tests/voc_stream_ops_lib.py) on the same inputs: for every stream of the batch the appended cache rows, the rotated q
and the output rows must be BIT-equal to what the single-stream launch gives.  tests/test_gpu_voc_stream_ops.py ties
the single-stream kernels to the whole-sequence attention and to the float64 reference; bit equality carries that over.

One batch of six streams (P, n) = (0, 1), (0, 33), (63, 2), (64, 1), (31, 70), (100, 4): an empty cache, a key-chunk
edge approached and crossed, three chunks from an unaligned P, tile counts 1, 2, 1, 1, 3, 1 (so most workgroups of the
(3, heads, 6) grid take the early exit).  The streams' caches are layer 1 of two-layer caches (the descriptor's layer
stride), each with 37 rows past P + n that are NaN sentinels in one run and zeros in another; guard rows surround each
stream's slice of the packed qkv and output.  The batch also runs with its descriptors in reversed order.
"""
import numpy as np
import pytest

import voc_stream_batch_ops_lib
import voc_stream_ops_lib
import voc_stream_ops_ref as S

pytestmark = pytest.mark.gpu

STREAMS = ((0, 1), (0, 33), (63, 2), (64, 1), (31, 70), (100, 4))   # (P, n)
EXTRA = 37                    # cache rows past P + n
SENT = np.uint32(0x7FC00123)  # a NaN
G = 5                         # guard rows around each stream's rows in the packed buffers
GUARD16 = np.uint16(0x7E01)
LAYER = 1


@pytest.fixture(scope="module")
def ops1():
    return voc_stream_ops_lib.load()


@pytest.fixture(scope="module")
def opsb():
    return voc_stream_batch_ops_lib.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_single = {}


def single(ops1, nH):
    """per stream, from the single-stream launchers (computed once per head count, never modified): the cache rows
    0..P-1 that earlier pushes left (k, v bits), the new rows before the append, and the launch results: qkv rows
    after the append, cache rows P..P+n-1 (k, v bits), output rows (f16 bits)"""
    if nH in _single:
        return _single[nH]
    LC = nH * 64
    res = []
    for P, n in STREAMS:
        qkv, rope = S.case(P, n, nH)
        F = P + n
        kc = np.full((F + EXTRA, LC), SENT, np.uint32)
        vc = np.full((F + EXTRA, LC), SENT, np.uint32)
        kd, vd, rd = ops1.DevBuf(kc), ops1.DevBuf(vc), ops1.DevBuf(rope)
        if P:   # the history: one push of the first P rows
            hd = ops1.DevBuf(np.ascontiguousarray(qkv[:P]))
            ops1.call("kv_append", hd.p, rd.p, kd.p, vd.p, 0, P, nH, 64)
        hist_k = kd.get(np.uint32, kc.size).reshape(kc.shape)[:P].copy()
        hist_v = vd.get(np.uint32, vc.size).reshape(vc.shape)[:P].copy()
        new = np.ascontiguousarray(qkv[P:])
        nd = ops1.DevBuf(new)
        ops1.call("kv_append", nd.p, rd.p, kd.p, vd.p, P, n, nH, 64)
        od = ops1.DevBuf(np.zeros((n, LC), np.uint16))
        ops1.call("attn_cached", nd.p, kd.p, vd.p, od.p, P, n, nH, 64)
        r = dict(P=P, n=n, rope=rope, new=new, hist_k=hist_k, hist_v=hist_v,
                 new_after=bits(nd.get(np.float32, new.size)).reshape(n, 3 * LC),
                 k_rows=kd.get(np.uint32, kc.size).reshape(kc.shape)[P:F].copy(),
                 v_rows=vd.get(np.uint32, vc.size).reshape(vc.shape)[P:F].copy(),
                 out=od.get(np.uint16, n * LC).reshape(n, LC))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        res.append(r)
    _single[nH] = res
    return res


def run_batch(opsb, ref, nH, fill, order):
    """one batched append + one batched attention over the six streams; returns per stream (in STREAMS order)
    (qkv rows after, k cache after, v cache after, out rows) and asserts that nothing else was written"""
    LC = nH * 64
    row0, at = [], G
    for r in ref:
        row0.append(at)
        at += r["n"] + G
    rows = at
    rng = np.random.default_rng(5)
    qkv = rng.standard_normal((rows, 3 * LC), dtype=np.float32)   # guard rows: values that must stay
    for r, r0 in zip(ref, row0):
        qkv[r0:r0 + r["n"]] = r["new"].reshape(r["n"], 3 * LC)
    out = np.full((rows, LC), GUARD16, np.uint16)
    qd, od = opsb.DevBuf(qkv), opsb.DevBuf(out)
    caches, items, keep = [], [], []
    for r in ref:
        P, n = r["P"], r["n"]
        R = P + n + EXTRA
        kc = np.full((2, R, LC), fill, np.uint32)     # layer 0 stays as it is: the launch works on layer 1
        vc = np.full((2, R, LC), fill, np.uint32)
        kc[LAYER, :P] = r["hist_k"]
        vc[LAYER, :P] = r["hist_v"]
        kd, vd, rd = opsb.DevBuf(kc), opsb.DevBuf(vc), opsb.DevBuf(r["rope"])
        keep += [kd, vd, rd]
        caches.append((kc, vc, kd, vd))
    for j in order:
        r = ref[j]
        _, _, kd, vd = caches[j]
        items.append((kd.p, vd.p, keep[3 * j + 2].p, (r["P"] + r["n"] + EXTRA) * LC, r["P"], r["n"], row0[j]))
    descs = opsb.descs(items)
    opsb.call("kv_append_batch", qd.p, descs, len(items), LAYER, nH, 64)
    qkv_after = qd.get(np.float32, qkv.size).reshape(qkv.shape)
    opsb.call("attn_cached_batch", qd.p, od.p, descs, len(items), LAYER, nH, 64)
    out_after = od.get(np.uint16, out.size).reshape(out.shape)
    assert np.array_equal(bits(qd.get(np.float32, qkv.size)), bits(qkv_after).ravel()), "the attention wrote qkv"
    touched_q = np.zeros(rows, bool)
    got = []
    for r, r0, (kc, vc, kd, vd) in zip(ref, row0, caches):
        P, n = r["P"], r["n"]
        F = P + n
        touched_q[r0:r0 + n] = True
        ka = kd.get(np.uint32, kc.size).reshape(kc.shape)
        va = vd.get(np.uint32, vc.size).reshape(vc.shape)
        for nm, before, after in (("K", kc, ka), ("V", vc, va)):
            assert np.array_equal(after[0], before[0]), f"{nm} cache of another layer written"
            assert np.array_equal(after[LAYER, :P], before[LAYER, :P]), f"{nm} cache rows before P changed"
            assert np.array_equal(after[LAYER, F:], before[LAYER, F:]), f"{nm} cache rows past P + n written"
        got.append((bits(qkv_after[r0:r0 + n]), ka[LAYER, P:F], va[LAYER, P:F], out_after[r0:r0 + n]))
    assert np.array_equal(bits(qkv_after[~touched_q]), bits(qkv[~touched_q])), "guard rows of qkv written"
    assert (out_after[~touched_q] == GUARD16).all(), "guard rows of the output written"
    return got


@pytest.mark.parametrize("nH", S.HEADS)
def test_batched_launches_match_the_single_stream_launchers(ops1, opsb, nH):
    ref = single(ops1, nH)
    fwd = list(range(len(STREAMS)))
    runs = {(fill, tuple(order)): run_batch(opsb, ref, nH, np.uint32(fill), order)
            for fill in (SENT, 0) for order in (fwd, fwd[::-1])}
    for key, got in runs.items():
        for r, (q_after, k_rows, v_rows, out) in zip(ref, got):
            tag = f"stream P={r['P']} n={r['n']} (fill {key[0]:#x}, order {key[1]})"
            assert np.array_equal(q_after, r["new_after"]), f"{tag}: qkv rows after the append differ"
            assert np.array_equal(k_rows, r["k_rows"]), f"{tag}: appended K rows differ"
            assert np.array_equal(v_rows, r["v_rows"]), f"{tag}: appended V rows differ"
            assert np.array_equal(out, r["out"]), f"{tag}: output rows differ from the single-stream launch"
            assert np.isfinite(out.view(np.float16).astype(np.float32)).all(), f"{tag}: a sentinel reached the output"
            assert np.isfinite(q_after.view(np.float32)).all() and np.isfinite(k_rows.view(np.float32)).all()
            assert np.isfinite(v_rows.view(np.float32)).all()


def test_copy_batch_moves_exactly_its_ranges(opsb):
    """voc_copy_batch: copies of different lengths in one launch (16-byte and 4-byte forms), bytes exact, nothing
    outside the destinations written"""
    rng = np.random.default_rng(9)
    for lens, shift in (((4, 1024, 4096 + 8, 70 * 1024), 0), ((3, 1, 1025, 5000), 1)):
        src = rng.standard_normal(sum(lens) + 64, dtype=np.float32)
        dst = np.full(sum(lens) + 16 * (len(lens) + 1) + 8, np.float32(-7.0))
        sd, dd = opsb.DevBuf(src), opsb.DevBuf(dst)
        copies, want, so, do = [], dst.copy(), shift, 16 + shift
        for n in lens:
            copies.append((sd.p + 4 * so, dd.p + 4 * do, n))
            want[do:do + n] = src[so:so + n]
            so += n
            do += n + 16
        opsb.copy_batch(copies[::-1])
        assert np.array_equal(bits(dd.get(np.float32, dst.size)), bits(want))
