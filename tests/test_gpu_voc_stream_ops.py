"""The vocoder stream's two kernels alone (k_voc_kv_append, k_voc_attn_cached), through the test-only shim
tests/voc_stream_ops/libq3t_voc_stream_ops.so, against

  * the whole-sequence attention q3t_ops_attn_prefill (tests/ops/) on the same P + n frames: the appended cache rows,
    the rotated q and the output rows P .. P+n-1 must be BIT-equal -- the property the stream's bit-exact PCM rests on;
  * the float64 reference of tests/voc_stream_ops_ref.py, within its CPU-derived tolerance.

Cases (voc_stream_ops_ref.CASES x HEADS): an empty cache, a key-chunk boundary approached and crossed by one- and
two-row pushes (P = 63, 64), and a push spanning three key chunks from an unaligned P.  The cache has rows past P + n:
they are sentinels (NaN) in one run and zeros in another; neither may reach a result, and the append may write only
rows P .. P+n-1.

Measured on an MI355X (every case prints its figures): the kernel's need_C is at most 0.02 against C_TOL_STREAM 1.59
(the CPU float32 re-evaluation needs 0.395); worst |err| / tol 0.98, which is the f16 half-ulp of the output itself.
"""
import numpy as np
import pytest

import voc_ops_lib
import voc_ops_ref as R
import voc_stream_ops_lib
import voc_stream_ops_ref as S

pytestmark = pytest.mark.gpu

EXTRA = 37                    # cache rows past P + n
SENT = np.uint32(0x7FC00123)  # a NaN
G = 8                         # guard rows around the output


@pytest.fixture(scope="module")
def whole_ops():
    return voc_ops_lib.load()


@pytest.fixture(scope="module")
def ops():
    return voc_stream_ops_lib.load()


def whole_sequence(whole_ops, qkv, rope, nH):
    """attn_prefill over all F frames: (rotated q [F][nH][64], rotated k, out bits [F][nH*64])"""
    F = qkv.shape[0]
    qd, rd = whole_ops.DevBuf(qkv), whole_ops.DevBuf(rope)
    od = whole_ops.DevBuf(np.zeros((F, nH * 64), np.uint16))
    whole_ops.call("attn_prefill", qd.p, rd.p, od.p, F, nH, 64, 1)
    after = qd.get(np.float32, qkv.size).reshape(qkv.shape)
    return after[:, 0], after[:, 1], od.get(np.uint16, F * nH * 64).reshape(F, nH * 64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("nH", S.HEADS)
@pytest.mark.parametrize("P,n", S.CASES)
def test_append_and_cached_attention(ops, whole_ops, P, n, nH):
    qkv, rope = S.case(P, n, nH)
    F, LC = P + n, nH * 64
    q_rot, k_rot, out_whole = whole_sequence(whole_ops, qkv, rope, nH)
    results = []
    for tail_fill in (SENT, np.uint32(0)):
        # the cache as P earlier pushes left it, unwritten rows behind
        kc = np.full((F + EXTRA, LC), tail_fill, np.uint32)
        vc = np.full((F + EXTRA, LC), tail_fill, np.uint32)
        kc[:P] = bits(k_rot[:P]).reshape(P, LC)
        vc[:P] = bits(qkv[:P, 2]).reshape(P, LC)
        kd, vd = ops.DevBuf(kc), ops.DevBuf(vc)
        new = np.ascontiguousarray(qkv[P:])
        nd, rd = ops.DevBuf(new), ops.DevBuf(rope)
        ops.call("kv_append", nd.p, rd.p, kd.p, vd.p, P, n, nH, 64)
        new_after = nd.get(np.float32, new.size).reshape(new.shape)
        kc_after = kd.get(np.uint32, kc.size).reshape(kc.shape)
        vc_after = vd.get(np.uint32, vc.size).reshape(vc.shape)
        # appended rows: k_rope_qk's bits; v copied; the rows before P and past P + n untouched
        assert np.array_equal(bits(new_after[:, 0]), bits(q_rot[P:])), "q not rotated as k_rope_qk rotates it"
        assert np.array_equal(bits(new_after[:, 1:]), bits(new[:, 1:])), "k / v columns of the new rows changed"
        assert np.array_equal(kc_after[P:F], bits(k_rot[P:]).reshape(n, LC)), "appended K rows differ from k_rope_qk"
        assert np.array_equal(vc_after[P:F], bits(qkv[P:, 2]).reshape(n, LC)), "appended V rows differ"
        assert np.array_equal(kc_after[:P], kc[:P]) and np.array_equal(vc_after[:P], vc[:P]), "cache rows before P changed"
        assert np.array_equal(kc_after[F:], kc[F:]) and np.array_equal(vc_after[F:], vc[F:]), "cache rows past P + n written"
        # attention over the cache
        out = np.full((G + n + G, LC), 0x7E01, np.uint16)
        od = ops.DevBuf(out)
        ops.call("attn_cached", nd.p, kd.p, vd.p, od.p + G * LC * 2, P, n, nH, 64)
        got = od.get(np.uint16, out.size).reshape(out.shape)
        assert (got[:G] == 0x7E01).all() and (got[G + n:] == 0x7E01).all(), "written outside the n output rows"
        results.append(got[G:G + n])
    got = results[0]
    assert np.array_equal(results[0], results[1]), "cache rows at or past P + n reached the output"
    vals = got.view(np.float16).astype(np.float64).reshape(n, nH, 64)
    assert np.isfinite(vals).all()
    assert np.array_equal(got, out_whole[P:]), "rows P..P+n-1 differ from the whole-sequence attention's bits"
    # values: from the f32 q / k the kernel itself read
    ref, allow = S.attention_rows(q_rot[P:].astype(np.float64), k_rot.astype(np.float64), qkv[:, 2].astype(np.float64), P)
    worst = R.worst_ratio(vals, ref, S.tol(ref, allow))
    need = R.need_c(vals, ref, S.U * allow, 2.0 ** -11 * np.abs(ref) + 2.0 ** -25)
    print(f"attn_cached P={P} n={n} nH={nH}: worst |err| / tol {worst:.3f}, need_C {need:.3f} (C_TOL_STREAM {S.C_TOL_STREAM})")
    assert worst <= 1
    # and the rotation's values (the bit comparison above ties it to k_rope_qk; this ties it to the formula)
    d = qkv[P:].astype(np.float64)
    r64 = rope[P:].astype(np.float64)
    for nm, gotr, j in (("q", new_after[:, 0], 0), ("k", kc_after[P:F].view(np.float32).reshape(n, nH, 64), 1)):
        mag = np.abs(np.concatenate([d[:, j, :, :32]] * 2, -1)) + np.abs(np.concatenate([d[:, j, :, 32:]] * 2, -1))
        assert R.worst_ratio(gotr, R.rope_neox(d[:, j], r64), 4 * S.U * mag) <= 1, f"RoPE of {nm}"
