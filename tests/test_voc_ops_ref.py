"""The references and the tolerance model of tests/voc_ops_ref.py, checked without a GPU: the two forms of the
transposed conv agree, the causal conv is numpy's, the tolerance model accepts a float32 evaluation of every operation
in another summation order -- and rejects four planted errors of the kinds a tiled kernel makes."""
import numpy as np
import pytest

import voc_ops_ref as R

U = R.U


def rnd16(rng, shape, sd=1.0):
    return R.f16(rng.standard_normal(shape) * sd)


def conv_case(rng, T, C_in, C_out, k):
    return rnd16(rng, (T, C_in)), rnd16(rng, (k, C_out, C_in), 1.0 / np.sqrt(k * C_in))


def conv_f32(x, w, pad, dil, M, gather=None, taps=None):
    """the causal conv in float32, taps and 32-channel chunks in the reverse of the reference's order.  gather(j, rows)
    returns the input rows of tap j (the hook the planted errors use)"""
    k, C_in = w.shape[0], w.shape[2]
    xp = np.concatenate([np.zeros((pad, C_in)), x, np.zeros((max(0, M + (k - 1) * dil - x.shape[0] - pad), C_in))], 0)
    rows = np.arange(M)
    acc = np.zeros((M, w.shape[1]), np.float32)
    for j in reversed(range(k) if taps is None else taps):
        xj = (xp[rows + j * dil] if gather is None else gather(j, rows, xp)).astype(np.float32)
        wj = w[j].astype(np.float32)
        for c0 in reversed(range(0, C_in, 32)):
            acc += xj[:, c0:c0 + 32] @ wj[:, c0:c0 + 32].T
    return acc


@pytest.mark.parametrize("k,st,trim", [(16, 8, 8), (10, 5, 5), (8, 4, 4), (6, 3, 3), (2, 2, 0)])
def test_transposed_scatter_equals_gather(k, st, trim):
    rng = np.random.default_rng(k)
    for T in (1, 2, 7):
        x, w = rnd16(rng, (T, 8)), rnd16(rng, (k, 5, 8))
        y, s = R.transposed_conv(x, w, st, trim)
        g = R.transposed_conv_gather(x, w, st, trim)
        assert y.shape == g.shape == (max((T - 1) * st + k - 2 * trim, 0), 5)
        np.testing.assert_allclose(y, g, rtol=0, atol=1e-12)
        assert np.all(s >= np.abs(y) - 1e-12)
        if len(y):   # a row subset is the same rows
            rows = np.unique([0, len(y) - 1, len(y) // 2])
            np.testing.assert_array_equal(R.transposed_conv(x, w, st, trim, rows=rows)[0], y[rows])


def test_causal_conv_is_numpy_convolve():
    rng = np.random.default_rng(1)
    T, C_in, C_out, k, dil = 9, 3, 2, 3, 2
    x, w = rnd16(rng, (T, C_in)), rnd16(rng, (k, C_out, C_in))
    pad = (k - 1) * dil
    y, _ = R.causal_conv(x, w, pad, dil)
    assert y.shape == (T, C_out)
    for co in range(C_out):
        want = np.zeros(T)
        for ci in range(C_in):
            kern = np.zeros(pad + 1)          # correlation with taps at j*dil = convolution with the flipped kernel
            kern[::dil] = w[::-1, co, ci]
            want += np.convolve(x[:, ci], kern)[:T]
        np.testing.assert_allclose(y[:, co], want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(R.causal_conv(x, w, pad, dil, rows=np.array([0, 4, 8]))[0], y[[0, 4, 8]])


def test_gelu_branches():
    x = np.array([-11.0, -10.0, -9.99, -1.0, 0.0, 0.5, 3.0, 9.99, 10.0, 12.3456789])
    g = R.gelu_ggml(x)
    assert g[0] == 0 and g[1] == 0 and g[-2] == 10.0 and g[-1] == 12.3456789
    assert np.all(g[2:-2] == R.f16(g[2:-2]))
    assert np.all(np.abs(g - R.gelu_smooth(x)) <= R.act_tol(0.0, x, 4))


# ------------------------------------------------------------------------------------------------ float32 accepted
@pytest.mark.parametrize("C_in,k,dil", [(96, 1, 1), (96, 7, 3), (192, 7, 9), (768, 7, 1)])
def test_f32_conv_accepted(C_in, k, dil):
    rng = np.random.default_rng(C_in + k)
    T, C_out = 200, 96
    x, w = conv_case(rng, T, C_in, C_out, k)
    bias, scale, resid = rng.standard_normal(C_out), np.exp(rng.standard_normal(C_out) * 0.3), rng.standard_normal((T, C_out))
    pad = (k - 1) * dil
    ref, s = R.causal_conv(x, w, pad, dil)
    acc = conv_f32(x, w, pad, dil, T)
    raw = R.worst_ratio(acc, ref, U * s)
    print(f"f32 conv n={C_in * k}: worst |err| / (u S_abs) = {raw:.2f}")
    assert raw < R.C_TOL_CONV / 4 + 1e-9, "the CPU figure behind C_TOL_CONV no longer holds"
    b32, s32, r32 = bias.astype(np.float32), scale.astype(np.float32), resid.astype(np.float32)
    v = (acc + b32) * s32 + r32
    b, sc, rs = b32.astype(np.float64), s32.astype(np.float64), r32.astype(np.float64)
    vref = (ref + b) * sc + rs
    dv = R.lin_tol(R.C_TOL_CONV, s, vref, b, sc, rs)
    assert R.worst_ratio(v, vref, dv) <= 1
    for act in (1, 2, 3, 4):
        got = {1: np.tanh(v), 2: np.maximum(v, 0), 3: np.tanh(np.maximum(v, 0)), 4: R.gelu_ggml(v)}[act]
        aref = R.act_apply(vref, act)
        da = R.act_tol(R.lin_tol(R.C_TOL_CONV, s, aref, b, sc, rs), vref, act)
        assert R.worst_ratio(got, aref, da) <= 1, act
    a, ib = (np.exp(rng.standard_normal(C_out) * 0.3).astype(np.float32) for _ in range(2))
    got16 = R.f16(v + ib * np.sin(a * v) ** 2)      # float32 arithmetic, rounded to f16
    a, ib = a.astype(np.float64), ib.astype(np.float64)
    assert R.worst_ratio(got16, R.snake(vref, a, ib), R.f16_tol(dv, R.snake(vref, a, ib), a, ib)) <= 1
    assert R.worst_ratio(R.f16(v), vref, R.f16_tol(dv, vref)) <= 1


def test_f32_transposed_accepted():
    rng = np.random.default_rng(5)
    T, C_in, C_out, K, st, trim = 40, 192, 96, 6, 3, 3
    x, w = rnd16(rng, (T, C_in)), rnd16(rng, (K, C_out, C_in), 1 / np.sqrt(2 * C_in))
    ref, s = R.transposed_conv(x, w, st, trim)
    got = np.zeros(ref.shape, np.float32)
    x32, w32 = x.astype(np.float32), w.astype(np.float32)
    for o in range(len(ref)):                        # gather form, float32
        m, phi = divmod(o, st)
        for kk in range((phi + trim) % st, K, st):
            i = m + (phi + trim - kk) // st
            if 0 <= i < T:
                got[o] += w32[kk] @ x32[i]
    assert R.worst_ratio(got, ref, R.lin_tol(R.C_TOL_CONV, s, ref)) <= 1


def test_f32_resunit_accepted():
    rng = np.random.default_rng(6)
    T, C, dil = 150, 96, 3
    xh, x = rnd16(rng, (T, C)), rng.standard_normal((T, C)).astype(np.float32)
    w1, w2 = rnd16(rng, (7, C, C), 1 / np.sqrt(7 * C)), rnd16(rng, (C, C), 1 / np.sqrt(C))
    b1, b2 = (rng.standard_normal(C).astype(np.float32) * 0.1 for _ in range(2))
    a2, ib2, an, ibn = (np.exp(rng.standard_normal(C) * 0.3).astype(np.float32) for _ in range(4))
    f32 = np.float32
    v1 = conv_f32(xh, w1, 6 * dil, dil, T) + b1
    h = R.f16(v1 + ib2 * np.sin(a2 * v1) ** 2)
    xo = x + (conv_f32(h, w2[None], 0, 1, T) + b2)
    assert xo.dtype == f32
    y16 = R.f16(xo + ibn * np.sin(an * xo) ** 2)
    d = [v.astype(np.float64) for v in (x, b1, a2, ib2, b2, an, ibn)]
    xr, yr, dx = R.resunit(xh, d[0], w1, d[1], d[2], d[3], w2, d[4], d[5], d[6], dil, R.C_TOL_CONV)
    assert R.worst_ratio(xo, xr, dx) <= 1
    assert R.worst_ratio(y16, yr, R.f16_tol(dx, yr, d[5], d[6])) <= 1


def test_f32_valu_ops_accepted():
    rng = np.random.default_rng(7)
    # depthwise conv and the single-channel output conv
    x, w, b = rng.standard_normal((50, 64)).astype(np.float32), rnd16(rng, (64, 7), 0.4), rng.standard_normal(64).astype(np.float32)
    ref, s = R.dwconv(x.astype(np.float64), w, b.astype(np.float64))
    got = np.zeros((50, 64), np.float32)
    xp = np.concatenate([np.zeros((6, 64)), R.f16(x)], 0).astype(np.float32)
    for j in range(7):
        got += xp[j:j + 50] * w[:, j].astype(np.float32)
    raw = R.worst_ratio(got, ref - b, U * s)
    got += b
    assert R.worst_ratio(got, ref, R.lin_tol(R.C_TOL_VALU, s, ref, b.astype(np.float64))) <= 1
    xh, w1 = rnd16(rng, (300, 96)), rnd16(rng, (7, 96), 1 / np.sqrt(7 * 96))
    y, v, s1 = R.conv_out1(xh, w1, 0.25)
    acc = conv_f32(xh, w1[:, None, :], 6, 1, 300)[:, 0]
    raw = max(raw, R.worst_ratio(acc, v - 0.25, U * s1))
    print(f"f32 VALU ops: worst |err| / (u S_abs) = {raw:.2f}")
    assert raw < R.C_TOL_VALU / 4 + 1e-9
    assert R.worst_ratio(np.tanh(acc + np.float32(0.25)), y, R.lin_tol(R.C_TOL_VALU, s1, y, 0.25)) <= 1
    # norms (one row with a large mean) and the snake pass
    for mode in (0, 1):
        x = rng.standard_normal((20, 512)).astype(np.float32)
        x[3] += np.float32(6.0)
        wn, bn = (rng.standard_normal(512).astype(np.float32) for _ in range(2))
        ref, mag, mm = R.norm_rows(x.astype(np.float64), wn.astype(np.float64), bn.astype(np.float64), 1e-5, mode)
        if mode == 0:
            got = x * (1 / np.sqrt((x.astype(np.float64) ** 2).mean(-1, keepdims=True) + 1e-5)).astype(np.float32) * wn
        else:
            d = x.astype(np.float64) - x.astype(np.float64).mean(-1, keepdims=True)
            got = d.astype(np.float32) * (1 / np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5)).astype(np.float32) * wn + bn
        assert got.dtype == np.float32
        assert R.worst_ratio(R.f16(got), ref, R.norm_tol(ref, mag, mm)) <= 1, mode
    z = (rng.standard_normal((33, 96)) * np.linspace(0.2, 40, 33)[:, None]).astype(np.float32)
    a, ib = (np.exp(rng.standard_normal(96) * 0.3).astype(np.float32) for _ in range(2))
    ref = R.snake(z.astype(np.float64), a.astype(np.float64), ib.astype(np.float64))
    r = (z * a) * np.float32(0.15915494309189535)
    got = R.f16(z + np.sin(np.float32(2 * np.pi) * (r - np.rint(r))) ** 2 * ib)
    assert R.worst_ratio(got, ref, R.f16_tol(0.0, ref, a.astype(np.float64), ib.astype(np.float64))) <= 1


def test_f32_attention_accepted():
    rng = np.random.default_rng(8)
    F, nH = 70, 2
    qkv = rng.standard_normal((F, 3, nH, 64)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, (F, 32))
    rope = np.stack([np.cos(ang), np.sin(ang)], -1).reshape(F, 64).astype(np.float32)
    d = qkv.astype(np.float64)
    q, k = R.rope_neox(d[:, 0], rope.astype(np.float64)), R.rope_neox(d[:, 1], rope.astype(np.float64))
    ref, allow = R.attention(q, k, d[:, 2])
    q32, k32, v32 = q.astype(np.float32), k.astype(np.float32), qkv[:, 2]
    got = np.zeros((F, nH, 64), np.float32)
    for i in range(F):                                # row by row, float32, keys in reverse order
        for h in range(nH):
            sc = (k32[i::-1, h] @ q32[i, h]) * np.float32(0.125)
            p = np.exp(sc - sc.max())
            got[i, h] = (p[None] @ v32[i::-1, h])[0] / p.sum()
    assert got.dtype == np.float32
    assert R.worst_ratio(R.f16(got), ref, R.attn_tol(R.C_TOL_VALU, ref, allow)) <= 1


# ------------------------------------------------------------------------------------------------ planted errors
@pytest.fixture(scope="module")
def planted():
    """a two-utterance 7-tap conv (192 -> 96 channels, dil 3) whose utterances lie 70 rows apart in one buffer"""
    rng = np.random.default_rng(11)
    T, C_in, C_out, k, dil = 140, 192, 96, 7, 3
    buf = rnd16(rng, (2 * T + 70, C_in))
    _, w = conv_case(rng, T, C_in, C_out, k)
    x = buf[T + 70:]                                  # the second utterance
    ref, s = R.causal_conv(x, w, (k - 1) * dil, dil)
    return dict(T=T, k=k, dil=dil, pad=(k - 1) * dil, buf=buf, x=x, w=w, ref=ref, tol=R.lin_tol(32.0, s, ref))


def flagged(p, got):
    return np.abs(got - p["ref"]) > p["tol"]


def test_planted_none_accepted(planted):
    p = planted
    assert not flagged(p, conv_f32(p["x"], p["w"], p["pad"], p["dil"], p["T"])).any()


def test_planted_dropped_tap_rejected(planted):
    p = planted
    got = conv_f32(p["x"], p["w"], p["pad"], p["dil"], p["T"], taps=[0, 1, 2, 4, 5, 6])
    bad = flagged(p, got)
    assert bad[p["pad"]:].mean() > 0.999       # (rows whose dropped tap reads padding are right by accident)


def test_planted_wrong_chunk_rejected(planted):
    p = planted

    def gather(j, rows, xp):
        xj = xp[rows + j * p["dil"]].copy()
        if j == 2:
            xj[77, 8:16] = xp[78 + j * p["dil"], 8:16]     # one 8-channel chunk of one row from the next row
        return xj
    bad = flagged(p, conv_f32(p["x"], p["w"], p["pad"], p["dil"], p["T"], gather=gather))
    assert bad[77].mean() > 0.99 and not np.delete(bad, 77, 0).any()


def test_planted_shifted_row_rejected(planted):
    p = planted
    got = conv_f32(p["x"], p["w"], p["pad"], p["dil"], p["T"])
    got[100] = got[101]
    bad = flagged(p, got)
    assert bad[100].mean() > 0.99 and not np.delete(bad, 100, 0).any()


def test_planted_neighbour_rows_for_padding_rejected(planted):
    p = planted
    T, pad = p["T"], p["pad"]
    xp_wrong = np.concatenate([p["buf"][T + 70 - pad:T + 70], p["x"]], 0)    # the rows before the utterance, not zeros

    def gather(j, rows, xp):
        return xp_wrong[rows + j * p["dil"]]
    bad = flagged(p, conv_f32(p["x"], p["w"], pad, p["dil"], T, gather=gather))
    assert bad[:p["dil"]].mean() > 0.99 and not bad[pad:].any()
