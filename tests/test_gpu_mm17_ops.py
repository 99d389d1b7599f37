"""Op-level checks of the kernel shapes the 1.7B matrix-core path added, one launch each through the test-only shim
tests/mm17_ops/ against numpy: resid_norm on rows up to 2,048 wide, select_embed_norm on the H = 2,048 step embedding
and on the f32 projected-table source, and gemv routed to the MFMA GEMM for the SwiGLU epilogue at K = 2,048 and the
split-K slabs of K = 6,144.

What is exact and what is bounded:
  - the residual rows (x + slabs in slab order; gathered rows summed left to right) are float32 sums in a fixed order:
    compared bit for bit with the same float32 sums in numpy;
  - normalised rows are f16 roundings of a float32 evaluation: within 1 f16 ulp of the float64 norm of those rows;
  - GEMM outputs on f16-rounded inputs against float64: within 2x the error the K = 1,024 SwiGLU / nk = 12 slab
    instantiations (which the 0.6B shapes already launch) show against the same kind of reference in the same test.
"""
import numpy as np
import pytest

import mm17_ops_lib

pytestmark = pytest.mark.gpu
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    return mm17_ops_lib.load()


def _f16_ulp(y):
    return np.spacing(np.abs(y).astype(np.float16)).astype(np.float64)


def _norm64(x32, w):
    x = x32.astype(np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + EPS) * w.astype(np.float64)


def _check_xn(xn_bits, x32, w):
    y = _norm64(x32, w)
    got = xn_bits.view(np.float16).astype(np.float64).reshape(y.shape)
    assert (np.abs(got - y) <= _f16_ulp(y)).all(), float((np.abs(got - y) / _f16_ulp(y)).max())
    return y


# ---------------------------------------------------------------------------------------------- resid_norm
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("ksplit", [0, 2, 3])
@pytest.mark.parametrize("H", [1024, 1028, 2044, 2048])
def test_resid_norm(ops, H, ksplit, S):
    rng = np.random.default_rng(H * 16 + ksplit * 4 + S)
    w = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    for with_xin in (False, True):
        for with_side in (False, True):
            x0 = rng.standard_normal((S, H)).astype(np.float32)
            xin = rng.standard_normal((S, H)).astype(np.float32) if with_xin else None
            parts = (rng.standard_normal((max(ksplit, 1), S, H)) * 0.3).astype(np.float32)
            want = (xin if with_xin else x0).copy()
            for z in range(ksplit):
                want = want + parts[z]   # float32, slab order
            dx, dw = ops.DevBuf(x0), ops.DevBuf(w)
            dxin = ops.DevBuf(xin) if with_xin else None
            dparts = ops.DevBuf(parts) if ksplit else None
            dxn = ops.DevBuf(nbytes=S * H * 2)
            dside = ops.DevBuf(np.zeros((S, H), np.float32)) if with_side else None
            chunks = ops.call("resid_norm", dxin.p if dxin else 0, dx.p, dparts.p if dparts else 0, ksplit, dw.p, EPS,
                              dxn.p, dside.p if dside else 0, S, H)
            # rows up to 1,024 wide run the narrow instantiation (every 0.6B launch: unchanged), wider ones the wide form
            assert chunks == (1 if H <= 1024 else 2), (H, chunks)
            x_out = dx.get(np.float32, S * H).reshape(S, H)
            assert np.array_equal(x_out, want if (ksplit or with_xin) else x0), (H, ksplit, S, with_xin)
            y = _check_xn(dxn.get(np.uint16, S * H), want, w)
            if with_side:
                side = dside.get(np.float32, S * H).reshape(S, H).astype(np.float64)
                assert (np.abs(side - y) <= 4 * 2.0 ** -24 * np.abs(y)).all()   # ~6 float32 roundings, each 2^-24


def test_resid_norm_refuses_rows_wider_than_2048(ops):
    d = ops.DevBuf(np.zeros(4096, np.float32))
    rc, err = ops.raw("resid_norm", 0, d.p, 0, 0, d.p, EPS, d.p, 0, 1, 2052)
    assert rc == -1 and "unsupported shape" in err


# ---------------------------------------------------------------------------------------------- select_embed_norm
def _select_state(ops, S, V, step, done_slot, rng):
    logits = rng.standard_normal((S, V)).astype(np.float32)
    tokens = rng.integers(0, V, (S, 16)).astype(np.int32)
    frame = rng.integers(0, 4, S).astype(np.int32)
    done = np.full(S, -1, np.int32)
    done[done_slot] = 1   # a finished slot: no selection, keeps the token already in the table
    tok = logits.argmax(axis=1).astype(np.int32)
    want_tokens = tokens.copy()
    live = done < 0
    want_tokens[live, step + 1] = tok[live]
    return logits, tokens, frame, done, want_tokens, live


def test_select_embed_norm_f32_table_row(ops):
    """nt = 1 from the projected table: x = ftab[row0 + token], xn = its norm (H = 1,024)"""
    S, V, H, step, row0 = 5, 2048, 1024, 3, 7
    rng = np.random.default_rng(41)
    logits, tokens, frame, done, want_tokens, live = _select_state(ops, S, V, step, 2, rng)
    ftab = rng.standard_normal((row0 + V, H)).astype(np.float32)
    w = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    d = {k: ops.DevBuf(v) for k, v in dict(logits=logits, tokens=tokens, frame=frame, done=done, ftab=ftab, w=w,
                                            codes=np.full((S, 8, 16), -1, np.int32), utt=np.arange(S, dtype=np.uint64),
                                            x=np.zeros((S, H), np.float32)).items()}
    dxn = ops.DevBuf(nbytes=S * H * 2)
    ops.call("select_embed_norm", d["logits"].p, V, step, 0.0, d["tokens"].p, d["codes"].p, 8, d["frame"].p, d["done"].p,
             d["utt"].p, 1, step + 1, 0, 0, 0, 0, 0, 0, d["ftab"].p, row0, d["x"].p, dxn.p, d["w"].p, EPS, H, S)
    got_tokens = d["tokens"].get(np.int32, S * 16).reshape(S, 16)
    assert np.array_equal(got_tokens, want_tokens)
    codes = d["codes"].get(np.int32, S * 8 * 16).reshape(S, 8, 16)
    for b in range(S):
        assert codes[b, frame[b], step + 1] == (want_tokens[b, step + 1] if live[b] else -1)
    want_x = ftab[row0 + want_tokens[:, step + 1]]
    assert np.array_equal(d["x"].get(np.float32, S * H).reshape(S, H), want_x)
    _check_xn(dxn.get(np.uint16, S * H), want_x, w)


@pytest.mark.parametrize("H", [2048, 1024])
def test_select_embed_norm_step_embedding(ops, H):
    """nt = 16: the talker step embedding, 16 f16 rows (the selected token among them) + the trailing / pad f32 row,
    at the 1.7B talker's width (the wide form) and at 1,024 (the narrow form every 0.6B hand-off launches)"""
    S, V, step = 5, 256, 14
    rng = np.random.default_rng(43 + H)
    logits, tokens, frame, done, want_tokens, live = _select_state(ops, S, V, step, 4, rng)
    tabs = (rng.standard_normal((16, V, H)) * 0.5).astype(np.float16)
    tr_rows = 2
    tr = rng.standard_normal((S, tr_rows, H)).astype(np.float32)
    tr_len = np.array([0, 1, 2, 2, 2], np.int32)   # with frame in 0..3: both the trailing row and the pad row occur
    frame[:] = [0, 1, 1, 3, 0]
    pad = rng.standard_normal((S, H)).astype(np.float32)
    w = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    dtab = [ops.DevBuf(tabs[j]) for j in range(16)]
    d = {k: ops.DevBuf(v) for k, v in dict(logits=logits, tokens=tokens, frame=frame, done=done, w=w, tr=tr, tr_len=tr_len,
                                            pad=pad, codes=np.full((S, 8, 16), -1, np.int32),
                                            utt=np.arange(S, dtype=np.uint64), x=np.zeros((S, H), np.float32),
                                            tabs=np.array([t.p for t in dtab], np.uint64)).items()}
    dxn = ops.DevBuf(nbytes=S * H * 2)
    ops.call("select_embed_norm", d["logits"].p, V, step, 0.0, d["tokens"].p, d["codes"].p, 8, d["frame"].p, d["done"].p,
             d["utt"].p, 16, 0, 0, d["tabs"].p, d["tr"].p, d["tr_len"].p, tr_rows * H, d["pad"].p, 0, 0, d["x"].p, dxn.p,
             d["w"].p, EPS, H, S)
    assert np.array_equal(d["tokens"].get(np.int32, S * 16).reshape(S, 16), want_tokens)
    want_x = np.zeros((S, H), np.float32)
    for b in range(S):
        acc = tabs[0, want_tokens[b, 0]].astype(np.float32)
        for j in range(1, 16):
            acc = acc + tabs[j, want_tokens[b, j]].astype(np.float32)   # float32, left to right
        want_x[b] = acc + (tr[b, frame[b]] if frame[b] < tr_len[b] else pad[b])
    assert np.array_equal(d["x"].get(np.float32, S * H).reshape(S, H), want_x)
    _check_xn(dxn.get(np.uint16, S * H), want_x, w)


# ---------------------------------------------------------------------------------------------- gemv -> MFMA GEMM
def _swiglu_err(ops, K, N, B, seed):
    """max |out - float64| / max |float64| of the SwiGLU GEMM over f16-rounded inputs; asserts the call was routed to
    the matrix-core GEMM"""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    x = rng.standard_normal((B, K)).astype(np.float16)
    dW, dx = ops.DevBuf(W), ops.DevBuf(x)
    dout = ops.DevBuf(nbytes=B * (N // 2) * 2)
    assert ops.call("gemv", dW.p, N, K, B, dx.p, 3, dout.p, 0, N // 2, 0, 0) == 1, "not routed to the MFMA GEMM"
    got = dout.get(np.uint16, B * (N // 2)).view(np.float16).astype(np.float64).reshape(B, N // 2)
    y = x.astype(np.float64) @ W.astype(np.float64).T   # rows in 16-row blocks [gate16 | up16]
    y = y.reshape(B, N // 32, 2, 16)
    g, u = y[:, :, 0], y[:, :, 1]
    ref = (g / (1.0 + np.exp(-g)) * u).reshape(B, N // 2)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("B", [4, 33])
def test_gemm_swiglu_at_k2048(ops, B):
    base = _swiglu_err(ops, 1024, 128, B, 50 + B)
    err = _swiglu_err(ops, 2048, 128, B, 60 + B)
    print(f"SwiGLU GEMM B={B}: K=1024 err {base:.3g}, K=2048 err {err:.3g}")
    assert err <= 2 * base, (B, err, base)


def _slab_err(ops, K, ksplit, N, B, seed):
    """worst slab's max |slab - float64| / max |float64| of the split-K slabs of a PRO_F16 GEMM"""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    x = rng.standard_normal((B, K)).astype(np.float16)
    dW, dx = ops.DevBuf(W), ops.DevBuf(x)
    dparts = ops.DevBuf(nbytes=ksplit * B * N * 4)
    assert ops.call("gemv", dW.p, N, K, B, dx.p, 0, 0, 0, N, dparts.p, ksplit) == 1, "not routed to the MFMA GEMM"
    got = dparts.get(np.float32, ksplit * B * N).astype(np.float64).reshape(ksplit, B, N)
    ks = K // ksplit
    worst = 0.0
    for z in range(ksplit):
        ref = x[:, z * ks:(z + 1) * ks].astype(np.float64) @ W[:, z * ks:(z + 1) * ks].astype(np.float64).T
        worst = max(worst, float(np.abs(got[z] - ref).max() / np.abs(ref).max()))
    return worst


@pytest.mark.parametrize("ksplit", [2, 3])
def test_gemm_slabs_at_k6144(ops, ksplit):
    base = _slab_err(ops, 3072, 1, 64, 33, 70)   # one slab of 12 K chunks: the 0.6B down projection's instantiation
    err = _slab_err(ops, 6144, ksplit, 64, 33, 80 + ksplit)
    print(f"slab GEMM K=6144 ksplit={ksplit}: err {err:.3g}; K=3072 one slab err {base:.3g}")
    assert err <= 2 * base, (ksplit, err, base)
