"""The vocoder's kernels, one operation at a time, against the float64 references of tests/voc_ops_ref.py.

Every case runs one launcher of csrc/vocoder_kernels.h through the test-only shim tests/ops/libq3t_ops.so on buffers of
its own, asserts which kernel conv() chose for it (q3t::conv_kernel), and checks
  * values: every element (a row subset for the big-tile cases: first and last row tile, two rows around every
    multiple of 128 and the whole tap span around the first and last 16 and every 16th of them -- the whole span
    around all would be 9 rows of 10 at dilation 9 -- and 1,024 random rows; every row tile of every utterance and
    channel tile is asserted to contribute) against the
    reference within the derived tolerance of voc_ops_ref (lin_tol / act_tol / f16_tol / norm_tol / attn_tol);
  * canaries: outputs are filled with a NaN sentinel before the launch; every element the operation owns must be
    written, every other one (rows >= M, columns >= C_out of a wider ldy, 64 guard rows before and after, the gap
    rows between utterances) must still hold the sentinel;
  * utterance edges: batches put the utterances 70 rows apart in the input with the gap (and 70 rows before and after)
    filled with f16 1000.0, so a read across an utterance's edge is orders of magnitude over the bound.

Tolerance constants (voc_ops_ref.C_TOL_CONV / C_TOL_VALU), in units of u * S_abs with u = 2^-24: 4 x the larger of
  the float32 re-evaluation on the CPU (tests/test_voc_ops_ref.py):  convs 1.75 (n = 96 .. 5376: 1.75, 1.04, 0.73, 0.84);
                                                                     VALU ops 2.83
  the kernels on an MI355X, first green run (this file; every test prints its need_C, test_zz_measured the largest):
      convs 2.59 (k_conv_pd<2, 64, 7>, 192 -> 128 channels, dil 9, 3 utterances; the other MFMA cases 0.4 .. 2.0);
      VALU ops 3.17 (k_dwconv, C = 1024; k_conv_out1 <= 1.05, k_attn_prefill <= 0.07 of its allowance)
  => C_TOL_CONV = 4 x 2.59 = 10.4, C_TOL_VALU = 4 x 3.17 = 12.7 (both below 32, where one dropped term of 5,376 is
     still ~20 x over the bound).  The f16 outputs' worst |err| / tol sits near 0.98: that is the f16 half-ulp itself.
The GELU bound applies its slope 1.13 to the input's f16 half-ulp as well (1.13 (dv + hu_in) + hu_out) and compares
with the GELU without its two roundings: against the rounded form, an input within dv of an f16 rounding boundary
legitimately lands one whole f16 step away.  The residual unit rounds h to f16 on chip: voc_ops_ref.resunit bounds that
the same way (only elements within their own error of a rounding boundary may move, by one step).
LayerNorm: 16 u on |term| + |bias| (= |ref| unless the two cancel), plus one rounding of the f32 mean.
"""
import ctypes as C
import os

import numpy as np
import pytest

import voc_ops_ref as R
from voc_ops_lib import GENERIC, MT, PD, ConvDesc, ResDesc, load

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = R.U
G = 64                      # guard rows around every output
XG, XGAP = 70, 70           # poisoned rows around the input and between its utterances
SENT32, SENT16 = 0x7FC00123, 0x7E01
NEED = {"conv": 0.0, "valu": 0.0}


@pytest.fixture(scope="module")
def ops():
    return load()


# ------------------------------------------------------------------------------------------------ buffers
def h16(a):
    """float64 values that are exact f16 -> their bits"""
    return np.asarray(a).astype(np.float16).view(np.uint16)


def rnd16(rng, shape, sd=1.0):
    return R.f16(rng.standard_normal(shape, dtype=np.float32) * np.float32(sd))


def snake_prm(rng, n):
    return tuple(np.exp(rng.standard_normal(n) * 0.3).astype(np.float32) for _ in range(2))


class InBuf:
    """nb utterances of T rows x Cn, xbs rows apart, the rows around and between them poisoned with 1000.0"""

    def __init__(self, ops, utts, dtype, xbs=None):
        nb, T, Cn = len(utts), utts[0].shape[0], utts[0].shape[1]
        self.xbs = xbs or (T + XGAP if nb > 1 else T)
        host = np.full((XG + (nb - 1) * self.xbs + T + XG, Cn), 1000.0, dtype)
        for u, a in enumerate(utts):
            host[XG + u * self.xbs:XG + u * self.xbs + T] = a
        self.dev = ops.DevBuf(host)
        self.p = self.dev.p + XG * Cn * host.itemsize


class OutBuf:
    """nb utterances of `rows` rows x ld (the first `cols` columns owned), ybs rows apart, NaN sentinels everywhere;
    G guard rows before and after.  fill: values to preload into the owned elements (a residual that aliases y)"""

    def __init__(self, ops, nb, rows, cols, ld, f32, fill=None):
        self.nb, self.rows, self.cols, self.ld, self.f32 = nb, rows, cols, ld, f32
        self.ybs = rows + G + 13 if nb > 1 else rows
        self.dt, self.sent = (np.uint32, SENT32) if f32 else (np.uint16, SENT16)
        host = np.full((G + (nb - 1) * self.ybs + rows + G, ld), self.sent, self.dt)
        self.owned = np.zeros(host.shape, bool)
        for u in range(nb):
            self.owned[G + u * self.ybs:G + u * self.ybs + rows, :cols] = True
            if fill is not None:
                host[G + u * self.ybs:G + u * self.ybs + rows, :cols] = fill[u].astype(np.float32).view(np.uint32)
        self.filled = fill is not None
        self.dev = ops.DevBuf(host)
        self.p = self.dev.p + G * ld * host.itemsize
        self.shape = host.shape

    def fetch(self):
        """canaries, then the utterances' values [nb][rows][cols] as float64"""
        bits = self.dev.get(self.dt, self.shape[0] * self.shape[1]).reshape(self.shape)
        stray = (bits != self.sent) & ~self.owned
        assert not stray.any(), f"written outside the output: first at (row, col) {np.argwhere(stray)[0] - [G, 0]}"
        if not self.filled:
            miss = (bits == self.sent) & self.owned
            assert not miss.any(), f"not written: first at (row, col) {np.argwhere(miss)[0] - [G, 0]}"
        vals = bits.view(np.float32 if self.f32 else np.float16)
        return [vals[G + u * self.ybs:G + u * self.ybs + self.rows, :self.cols].astype(np.float64) for u in range(self.nb)]


def big_rows(M, tile, span, rng, nrand=1024):
    """the compared rows of a big-tile case: the first and last row tile, the rows within 2 of every multiple of 128
    (within the whole tap span of the first and last 16 and of every 16th: the reference's cost), and random rows"""
    if M <= 2048:
        return np.arange(M)
    mult = np.arange(0, M + 128, 128)
    wide = np.concatenate([mult[:16], mult[-16:], mult[::16]])
    near = np.concatenate([(mult[:, None] + np.arange(-2, 3)[None]).ravel(),
                           (wide[:, None] + np.arange(-span, span + 1)[None]).ravel()])
    rows = np.concatenate([np.arange(tile), np.arange((M - 1) // tile * tile, M), near, rng.integers(0, M, nrand)])
    rows = np.unique(rows[(rows >= 0) & (rows < M)])
    assert len(np.unique(rows // tile)) == (M + tile - 1) // tile, "a row tile without a compared row"
    return rows


def report(kind, name, ratio, need=None):
    if need is not None:
        NEED[kind] = max(NEED[kind], need)
    print(f"{name}: worst |err| / tol = {ratio:.3f}" + (f", need_C = {need:.2f}" if need is not None else ""))


# ------------------------------------------------------------------------------------------------ conv cases
OPTS = ["plain", "bias", "scale", "resid", "resid_alias", "act1", "act2", "act3", "act4", "y_only", "y16_only",
        "y16_snake", "ldy", "all"]


def run_conv(ops, rng, expect, C_in, C_out, k, dil, T, nb, opt="plain", ct=None, x_f32=False, act=0, env=None,
             name=""):
    """one conv launch (ct = (K, st, trim): transposed, every phase in one launch) checked against the reference.
    expect = (family, RB, NT, TW or TAPS, MINB); returns the worst |err| / tol"""
    has = lambda o: opt == o or (opt == "all" and o in ("bias", "scale", "resid_alias", "y16_snake", "ldy"))
    if opt in ("act1", "act2", "act3", "act4"):
        act = int(opt[3])
    elif opt == "all":
        act = 3
    want_y, want_y16 = opt != "y16_only", opt != "y_only"
    n = (2 if ct else k) * C_in
    if ct:
        K, st, trim = ct
        T_out = (T - 1) * st + K - 2 * trim
        w = rnd16(rng, (K, C_out, C_in), 1 / np.sqrt(n))
    else:
        pad, T_out = (k - 1) * dil, T
        w = rnd16(rng, (k, C_out, C_in), 1 / np.sqrt(n))
    rows_out = max(T_out, 1)
    # inputs: f16 rows, or f32 rows with the snake applied inside the kernel (generic kernel)
    sa = sib = None
    if x_f32:
        x32 = [rng.standard_normal((T, C_in), dtype=np.float32) for _ in range(nb)]
        sa, sib = snake_prm(rng, C_in)
        xin = InBuf(ops, x32, np.float32)
        xs, dxs = [], []
        for a in x32:   # the kernel's f16(snake(x)): elements within the sine's error of a rounding boundary may differ
            s = R.snake(a.astype(np.float64), sa.astype(np.float64), sib.astype(np.float64))
            hq, dh = R.f16_round_dev(s, 4e-6 * sib + 8 * U * np.abs(s))
            xs.append(hq), dxs.append(dh)
    else:
        xs = [rnd16(rng, (T, C_in)) for _ in range(nb)]
        xin = InBuf(ops, [h16(a) for a in xs], np.uint16)
    ldy = C_out + 32 if has("ldy") else C_out
    bias = (rng.standard_normal(C_out) * 0.5).astype(np.float32) if has("bias") else None
    scale = np.exp(rng.standard_normal(C_out) * 0.3).astype(np.float32) if has("scale") else None
    resid = None
    if has("resid") or has("resid_alias"):
        resid = [rng.standard_normal((rows_out, C_out), dtype=np.float32) for _ in range(nb)]
    ya = yib = None
    if has("y16_snake"):
        ya, yib = snake_prm(rng, C_out)
    ybuf = OutBuf(ops, nb, rows_out, C_out, ldy, True, fill=resid if has("resid_alias") else None) \
        if (want_y or has("resid_alias")) else None
    y16buf = OutBuf(ops, nb, rows_out, C_out, C_out, False) if want_y16 else None
    rbuf = None
    if has("resid") and not has("resid_alias"):
        rbuf = OutBuf(ops, nb, rows_out, C_out, ldy, True, fill=resid)
    if T_out == 0:   # nothing to write: the buffers keep one (never written) row
        for b in (ybuf, y16buf):
            if b is not None:
                b.owned[:] = False
    dev = {kk: ops.DevBuf(v) for kk, v in dict(w=h16(w), bias=bias, scale=scale, ya=ya, yib=yib, sa=sa, sib=sib).items()
           if v is not None}
    P = lambda kk: dev[kk].p if kk in dev else 0
    d = ConvDesc()
    if x_f32:
        d.x, d.snake_a, d.snake_ib = xin.p, P("sa"), P("sib")
    else:
        d.xh = xin.p
    d.T_in, d.C_in, d.C_out, d.ldy, d.act, d.nb = T, C_in, C_out, (ldy if has("ldy") else 0), act, nb
    d.y = ybuf.p if ybuf is not None else 0
    d.y16 = y16buf.p if y16buf is not None else 0
    d.y16_a, d.y16_ib, d.bias, d.scale = P("ya"), P("yib"), P("bias"), P("scale")
    d.resid = ybuf.p if has("resid_alias") else rbuf.p if rbuf is not None else 0
    d.xbs = xin.xbs
    d.ybs = (ybuf or y16buf).ybs
    assert y16buf is None or ybuf is None or y16buf.ybs == ybuf.ybs
    if ct:
        d.ct_w, d.ct_k, d.ct_st, d.ct_trim, d.T_out = P("w"), K, st, trim, T_out
    else:
        d.w, d.M, d.n_taps, d.dil, d.pad, d.so, d.ob = P("w"), T, k, dil, pad, 1, 0
    old = {kk: os.environ.get(kk) for kk in (env or {})}
    os.environ.update(env or {})
    try:
        got = ops.kernel(d)
        want = (0,) * 6 if T_out == 0 else tuple(expect) + (0 if expect[0] == GENERIC else 1,)
        assert got == want, f"conv() chose {got}, the case is meant for {want}"
        ops.call("conv", C.byref(d))
    finally:
        for kk, v in old.items():
            os.environ.pop(kk) if v is None else os.environ.__setitem__(kk, v)
    ys = ybuf.fetch() if ybuf is not None else None
    y16s = y16buf.fetch() if y16buf is not None else None
    if rbuf is not None:
        rbuf.fetch()    # (the residual is only read)
    if T_out == 0:
        return 0.0
    # ---- values
    c_tol = R.C_TOL_CONV
    tile = 128 * expect[1] if expect[0] != GENERIC else 64
    b64 = bias.astype(np.float64) if bias is not None else 0.0
    s64 = scale.astype(np.float64) if scale is not None else 1.0
    worst = need = 0.0
    for u in range(nb):
        if ct:
            mrows = big_rows((T_out + st - 1) // st, tile, 3, rng, 1024 // st)
            rows = (mrows[:, None] * st + np.arange(st)[None]).ravel()
            rows = rows[rows < T_out]
            acc, S = R.transposed_conv(xs[u], w, st, trim, rows=rows)
        else:
            rows = big_rows(T, tile, (k - 1) * dil + 2, rng)
            acc, S = R.causal_conv(xs[u], w, pad, dil, M=T, rows=rows)
            if x_f32:
                extra = R.causal_conv(dxs[u], np.abs(w), pad, dil, M=T, rows=rows)[0]
        r64 = resid[u][rows].astype(np.float64) if resid is not None else 0.0
        v = (acc + b64) * s64 + r64
        aref = R.act_apply(v, act)
        dv = R.lin_tol(c_tol, S, aref, b64, s64, r64)
        if x_f32:
            dv = dv + np.abs(s64) * extra
        da = R.act_tol(dv, v, act)
        if want_y:
            worst = max(worst, R.worst_ratio(ys[u][rows], aref, da))
            if act == 0 and not x_f32:
                need = max(need, R.need_c(ys[u][rows], aref, U * (np.abs(s64) * (S + np.abs(b64)) + np.abs(r64))))
        if want_y16:
            a64, i64 = (ya.astype(np.float64), yib.astype(np.float64)) if ya is not None else (0.0, 0.0)
            sref = R.snake(aref, a64, i64) if ya is not None else aref
            worst = max(worst, R.worst_ratio(y16s[u][rows], sref, R.f16_tol(da, sref, a64, i64)))
    report("conv", name or f"conv {expect} {C_in}->{C_out} k{k} dil{dil} T{T} nb{nb} {opt}", worst,
           need if (want_y and act == 0 and not x_f32) else None)
    return worst


def nt_of(C_out):
    return 96 if C_out % 96 == 0 else 64


@pytest.mark.parametrize("C_in", [32, 96])
@pytest.mark.parametrize("C_out", [64, 96, 128, 192])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_conv_mt_small(ops, C_in, C_out, k):
    """k_conv_mt<1, NT, 2, TW>: every dilation, M around the 128-row tile, batches, each epilogue option alone (in
    rotation over the shapes) and all together"""
    rng = np.random.default_rng(1000 * C_in + 10 * C_out + k)
    expect = (MT, 1, nt_of(C_out), k, 2)
    worst, i = 0.0, 0
    for dil in ((1,) if k == 1 else (1, 3, 9)):
        for M in (1, 127, 128, 129, 300):
            for nb in (1, 3):
                for opt in (OPTS[i % (len(OPTS) - 1)], "all"):
                    worst = max(worst, run_conv(ops, rng, expect, C_in, C_out, k, dil, M, nb, opt))
                i += 1
    for opt in OPTS:   # every option at one ragged two-tile shape
        worst = max(worst, run_conv(ops, rng, expect, C_in, C_out, k, 3 if k > 1 else 1, 129, 3, opt))
    assert worst <= 1


@pytest.mark.parametrize("Cn,nb", [(96, 2), (192, 1)])
def test_conv_mt_1tap_narrow(ops, Cn, nb):
    """k_conv_mt<1, NT, 3, 1>: the residual prefetch (rows clamped to M - 1) with the residual aliasing y, a ragged last
    tile and a row-tile count that is no multiple of 8 (the XCD order's short last group)"""
    rng = np.random.default_rng(Cn)
    M = 256 * 256 + 77 if Cn == 96 else 255 * 256 + 1 + 77      # tiles256 = 514 / 512
    assert run_conv(ops, rng, (MT, 1, 96, 1, 3), Cn, Cn, 1, 1, M, nb, "all") <= 1
    assert run_conv(ops, rng, (MT, 1, 96, 1, 3), Cn, Cn, 1, 1, M, nb, "resid_alias") <= 1


@pytest.mark.parametrize("C_out", [192, 128])
def test_conv_mt_7tap_big(ops, C_out):
    """k_conv_mt<2, 96, 2, 7> (the shape without weight prefetch) and <2, 64, 2, 7>, reached with Q3T_CONV_PD=0"""
    rng = np.random.default_rng(C_out)
    M = 255 * 256 + 1 + 77
    for dil, opt in ((3, "bias"), (9, "all")):
        assert run_conv(ops, rng, (MT, 2, nt_of(C_out), 7, 2), C_out, C_out, 7, dil, M, 1, opt,
                        env={"Q3T_CONV_PD": "0"}) <= 1


@pytest.mark.parametrize("C_out", [192, 128])
@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("nb", [1, 3])
def test_conv_pd(ops, C_out, dil, nb):
    """k_conv_pd<4, NT, 7> and, with Q3T_CONV_PD=1, <2, NT, 7>: M ragged against 256 and 512, the batch's padding
    taken from the buffer range check next to poisoned rows"""
    rng = np.random.default_rng(100 * C_out + 10 * dil + nb)
    M = (255 * 256 + 1 if nb == 1 else 85 * 256 + 1) + 77
    assert M % 256 and M % 512
    opt = ("bias", "all", "y16_snake")[(dil // 3 + nb) % 3]
    assert run_conv(ops, rng, (PD, 4, nt_of(C_out), 7, 1), 192, C_out, 7, dil, M, nb, opt) <= 1
    assert run_conv(ops, rng, (PD, 2, nt_of(C_out), 7, 1), 192, C_out, 7, dil, M, nb, opt, env={"Q3T_CONV_PD": "1"}) <= 1


@pytest.mark.parametrize("shape", [(192, 96, 6, 3), (384, 192, 8, 4)])
def test_conv_transposed_mt(ops, shape):
    C_in, C_out, K, st = shape
    rng = np.random.default_rng(K)
    for T in (1, 43, 129):
        for nb in (1, 3):
            for opt in ("bias", "y16_snake"):
                assert run_conv(ops, rng, (MT, 1, 96, 3, 2), C_in, C_out, 0, 0, T, nb, opt, ct=(K, st, K - st)) <= 1


@pytest.mark.parametrize("shape", [(1536, 768, 16, 8, 2051), (768, 384, 10, 5, 25 * 256 + 1 + 77 + 1)])
def test_conv_transposed_pd(ops, shape):
    """k_conv_pd<4, 96, 2>: every output phase in one launch, 512-row tiles with a ragged last one"""
    C_in, C_out, K, st, T = shape
    rng = np.random.default_rng(K)
    assert run_conv(ops, rng, (PD, 4, 96, 2, 1), C_in, C_out, 0, 0, T, 1, "y16_snake", ct=(K, st, K - st)) <= 1


def test_conv_per_phase(ops):
    """the per-phase path (so = st, ob = phi) as Vocoder::run_convT builds it: k 2, stride 2, no trim -> one 1-tap
    launch per output phase into the rows 2 m + phi of one output"""
    rng = np.random.default_rng(2)
    Cn, T, st, nb = 64, 129, 2, 3
    T_out = 2 * T
    w = rnd16(rng, (2, Cn, Cn), 1 / np.sqrt(Cn))
    bias = (rng.standard_normal(Cn) * 0.5).astype(np.float32)
    xs = [rnd16(rng, (T, Cn)) for _ in range(nb)]
    xin = InBuf(ops, [h16(a) for a in xs], np.uint16)
    ybuf = OutBuf(ops, nb, T_out, Cn, Cn, True)
    wd, bd = ops.DevBuf(h16(w)), ops.DevBuf(bias)
    for phi in range(st):
        d = ConvDesc()
        d.xh, d.T_in, d.C_in, d.C_out, d.nb, d.xbs, d.ybs = xin.p, T, Cn, Cn, nb, xin.xbs, ybuf.ybs
        d.w, d.n_taps, d.dil, d.pad = wd.p + phi * Cn * Cn * 2, 1, 1, 0      # tap k = phi at input offset 0
        d.M, d.so, d.ob, d.y, d.bias = (T_out - phi + st - 1) // st, st, phi, ybuf.p, bd.p
        assert ops.kernel(d) == (MT, 1, 64, 1, 2, 1)
        ops.call("conv", C.byref(d))
    worst = need = 0.0
    for u, y in enumerate(ybuf.fetch()):
        acc, S = R.transposed_conv(xs[u], w, st, 0)
        ref = acc + bias
        worst = max(worst, R.worst_ratio(y, ref, R.lin_tol(R.C_TOL_CONV, S, ref, bias)))
        need = max(need, R.need_c(y, ref, U * (S + np.abs(bias))))
    report("conv", "per-phase transposed", worst, need)
    assert worst <= 1


def test_conv_generic(ops):
    """k_conv: channel counts that are no multiple of 8 or 32 with f32 input and the snake inside the kernel, and the
    single-output-channel shape around its 64-row tile"""
    rng = np.random.default_rng(3)
    for T, nb in ((65, 1), (150, 3)):
        assert run_conv(ops, rng, (GENERIC, 0, 0, 0, 0), 20, 40, 3, 2, T, nb, "bias", x_f32=True, act=1) <= 1
    for M in (1, 64, 65):
        for C_in in (96, 100):     # (100: f16 rows that are no multiple of 8 channels)
            assert run_conv(ops, rng, (GENERIC, 0, 0, 0, 0), C_in, 1, 7, 1, M, 2, "bias", act=1) <= 1


# ------------------------------------------------------------------------------------------------ residual unit
@pytest.mark.parametrize("T", [1, 255, 256, 257, 600])
def test_resunit96(ops, T):
    rng = np.random.default_rng(T)
    Cn, worst = 96, 0.0
    w1, w2 = rnd16(rng, (7, Cn, Cn), 1 / np.sqrt(7 * Cn)), rnd16(rng, (Cn, Cn), 1 / np.sqrt(Cn))
    b1, b2 = ((rng.standard_normal(Cn) * 0.5).astype(np.float32) for _ in range(2))
    (a2, ib2), (an, ibn) = snake_prm(rng, Cn), snake_prm(rng, Cn)
    prm = [ops.DevBuf(v) for v in (h16(w1), h16(w2), b1, a2, ib2, b2, an, ibn)]
    f64 = [v.astype(np.float64) for v in (b1, a2, ib2, b2, an, ibn)]
    for dil in (1, 3, 9):
        for nb in (1, 3):
            xs = [rnd16(rng, (T, Cn)) for _ in range(nb)]
            x32 = [rng.standard_normal((T, Cn), dtype=np.float32) for _ in range(nb)]
            refs = [R.resunit(xs[u], x32[u].astype(np.float64), w1, f64[0], f64[1], f64[2], w2, f64[3], f64[4], f64[5],
                              dil, R.C_TOL_CONV) for u in range(nb)]
            for ymode in ("null", "alias", "separate"):
                # xh, x, y and y16 share one utterance stride: poisoned gap rows in the input, sentinels in the others
                y16buf = OutBuf(ops, nb, T, Cn, Cn, False)
                xbuf = OutBuf(ops, nb, T, Cn, Cn, True, fill=x32)
                ybuf = OutBuf(ops, nb, T, Cn, Cn, True) if ymode == "separate" else None
                bs = y16buf.ybs
                xin = InBuf(ops, [h16(a) for a in xs], np.uint16, xbs=bs)
                d = ResDesc()
                d.xh, d.x, d.y16, d.T, d.dil, d.nb, d.bs = xin.p, xbuf.p, y16buf.p, T, dil, nb, bs
                d.y = {"null": 0, "alias": xbuf.p, "separate": ybuf.p if ybuf else 0}[ymode]
                d.w1, d.w2, d.b1, d.a2, d.ib2, d.b2, d.an, d.ibn = (b.p for b in prm)
                ops.call("resunit96", C.byref(d))
                y16 = y16buf.fetch()
                xo = xbuf.fetch()
                yo = ybuf.fetch() if ybuf else None
                for u in range(nb):
                    xr, yr, dx = refs[u]
                    worst = max(worst, R.worst_ratio(y16[u], yr, R.f16_tol(dx, yr, f64[4], f64[5])))
                    if ymode == "alias":
                        worst = max(worst, R.worst_ratio(xo[u], xr, dx))
                    else:
                        assert np.array_equal(xo[u], x32[u].astype(np.float64)), "x changed"
                    if yo:
                        worst = max(worst, R.worst_ratio(yo[u], xr, dx))
    report("conv", f"resunit96 T={T}", worst)
    assert worst <= 1


# ------------------------------------------------------------------------------------------------ VALU ops
@pytest.mark.parametrize("Cn", [8, 96, 104])
@pytest.mark.parametrize("K", [1, 7, 8])
def test_conv_out1(ops, Cn, K):
    rng = np.random.default_rng(10 * Cn + K)
    worst = need = 0.0
    nb = 2
    for T in (1, 255, 256, 257, 1000):
        xs = [rnd16(rng, (T, Cn)) for _ in range(nb)]
        w = rnd16(rng, (K, Cn), 1 / np.sqrt(K * Cn))
        bias = np.float32(rng.standard_normal() * 0.5)
        host = np.full((XG + nb * T + XG, Cn), 1000.0, np.float16).view(np.uint16)     # utterances back to back
        for u in range(nb):
            host[XG + u * T:XG + (u + 1) * T] = h16(xs[u])
        xd, wd, bd = ops.DevBuf(host), ops.DevBuf(h16(w)), ops.DevBuf(np.array([bias], np.float32))
        ybuf = OutBuf(ops, 1, nb * T, 1, 1, True)
        ops.call("conv_out1", xd.p + XG * Cn * 2, wd.p, bd.p, ybuf.p, T, Cn, K, nb)
        y = ybuf.fetch()[0][:, 0]
        for u in range(nb):
            ref, v, S = R.conv_out1(xs[u], w, float(bias))
            worst = max(worst, R.worst_ratio(y[u * T:(u + 1) * T], ref, R.lin_tol(R.C_TOL_VALU, S, ref, float(bias))))
            need = max(need, R.need_c(y[u * T:(u + 1) * T], ref, U * (S + abs(float(bias))), 8 * U * np.abs(ref)))
    report("valu", f"conv_out1 C={Cn} K={K}", worst, need)
    assert worst <= 1


@pytest.mark.parametrize("Cn", [64, 1024])
def test_dwconv(ops, Cn):
    rng = np.random.default_rng(Cn)
    worst = need = 0.0
    nb, K = 2, 7
    for T in (1, 6, 300):
        x32 = [rng.standard_normal((T, Cn), dtype=np.float32) for _ in range(nb)]
        w = rnd16(rng, (Cn, K), 1 / np.sqrt(K))
        b = (rng.standard_normal(Cn) * 0.5).astype(np.float32)
        host = np.full((XG + nb * T + XG, Cn), 1000.0, np.float32)
        for u in range(nb):
            host[XG + u * T:XG + (u + 1) * T] = x32[u]
        xd, wd, bd = ops.DevBuf(host), ops.DevBuf(h16(w)), ops.DevBuf(b)
        ybuf = OutBuf(ops, 1, nb * T, Cn, Cn, True)
        ops.call("dwconv", xd.p + XG * Cn * 4, wd.p, bd.p, ybuf.p, T, Cn, K, nb)
        y = ybuf.fetch()[0]
        for u in range(nb):
            ref, S = R.dwconv(x32[u].astype(np.float64), w, b.astype(np.float64))
            worst = max(worst, R.worst_ratio(y[u * T:(u + 1) * T], ref, R.lin_tol(R.C_TOL_VALU, S, ref, b.astype(np.float64))))
            need = max(need, R.need_c(y[u * T:(u + 1) * T], ref, U * (S + np.abs(b))))
    report("valu", f"dwconv C={Cn}", worst, need)
    assert worst <= 1


@pytest.mark.parametrize("nH", [1, 16])
@pytest.mark.parametrize("nb", [1, 3])
def test_attn_prefill(ops, nH, nb):
    rng = np.random.default_rng(10 * nH + nb)
    worst = need = 0.0
    for F in (1, 31, 32, 33, 64, 65, 130):
        qkv = rng.standard_normal((nb, F, 3, nH, 64), dtype=np.float32)
        ang = rng.uniform(0, 2 * np.pi, (F, 32))
        rope = np.stack([np.cos(ang), np.sin(ang)], -1).reshape(F, 64).astype(np.float32)
        qd, rd = ops.DevBuf(qkv), ops.DevBuf(rope)
        obuf = OutBuf(ops, 1, nb * F, nH * 64, nH * 64, False)
        ops.call("attn_prefill", qd.p, rd.p, obuf.p, F, nH, 64, nb)
        out = obuf.fetch()[0].reshape(nb, F, nH, 64)
        after = qd.get(np.float32, qkv.size).reshape(qkv.shape)
        assert np.array_equal(after[:, :, 2], qkv[:, :, 2]), "v columns changed"
        r64 = rope.astype(np.float64)
        for u in range(nb):
            d = qkv[u].astype(np.float64)
            q, k = R.rope_neox(d[:, 0], r64), R.rope_neox(d[:, 1], r64)
            for nm, got, want in (("q", after[u, :, 0], q), ("k", after[u, :, 1], k)):
                mag = np.abs(np.concatenate([d[:, "qk".index(nm), :, :32]] * 2, -1)) + \
                      np.abs(np.concatenate([d[:, "qk".index(nm), :, 32:]] * 2, -1))
                assert R.worst_ratio(got, want, 4 * U * mag) <= 1, f"RoPE of {nm}"
            # the attention proper, from the f32 q / k the kernel itself read
            qa, ka = after[u, :, 0].astype(np.float64), after[u, :, 1].astype(np.float64)
            ref, allow = R.attention(qa, ka, d[:, 2])
            worst = max(worst, R.worst_ratio(out[u], ref, R.attn_tol(R.C_TOL_VALU, ref, allow)))
            need = max(need, R.need_c(out[u], ref, U * allow, 2.0 ** -11 * np.abs(ref) + 2.0 ** -25))
    report("valu", f"attn_prefill nH={nH} nb={nb}", worst, need)
    assert worst <= 1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Cn", [4, 96, 512, 1024])
def test_norm_f16(ops, mode, Cn):
    rng = np.random.default_rng(10 * Cn + mode)
    worst = 0.0
    for T in (1, 300):
        x = rng.standard_normal((T, Cn), dtype=np.float32)
        x[T // 2] += np.float32(6.0)       # one row with a large mean (LayerNorm's x - mean cancels)
        w, b = (rng.standard_normal(Cn).astype(np.float32) for _ in range(2))
        xd, wd, bd = ops.DevBuf(x), ops.DevBuf(w), ops.DevBuf(b)
        obuf = OutBuf(ops, 1, T, Cn, Cn, False)
        ops.call("norm_f16", xd.p, wd.p, bd.p if mode else 0, 1e-5, mode, obuf.p, T, Cn)
        ref, mag, mm = R.norm_rows(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), float(np.float32(1e-5)), mode)
        worst = max(worst, R.worst_ratio(obuf.fetch()[0], ref, R.norm_tol(ref, mag, mm)))
    report("valu", f"norm_f16 mode={mode} C={Cn}", worst)
    assert worst <= 1


@pytest.mark.parametrize("Cn", [4, 96])
@pytest.mark.parametrize("with_a", [False, True])
def test_snake_f16(ops, Cn, with_a):
    rng = np.random.default_rng(Cn)
    T = 1028 // 4 if Cn == 4 else 43          # T * C = 1028 / 4128: no multiple of 1024
    assert (T * Cn) % 1024 and (T * Cn) % 4 == 0
    a, ib = snake_prm(rng, Cn)
    z = (rng.standard_normal((T, Cn)) * np.linspace(0.2, 17, T)[:, None]).astype(np.float32)   # |a z| up to ~50
    zd, ad, ibd = ops.DevBuf(z), ops.DevBuf(a), ops.DevBuf(ib)
    obuf = OutBuf(ops, 1, T, Cn, Cn, False)
    ops.call("snake_f16", zd.p, ad.p if with_a else 0, ibd.p if with_a else 0, obuf.p, T, Cn)
    a64, i64 = (a.astype(np.float64), ib.astype(np.float64)) if with_a else (0.0, 0.0)
    ref = R.snake(z.astype(np.float64), a64, i64) if with_a else z.astype(np.float64)
    worst = R.worst_ratio(obuf.fetch()[0], ref, R.f16_tol(0.0, ref, a64, i64))
    report("valu", f"snake_f16 C={Cn} a={with_a} (max |a z| {np.abs(z * a).max():.0f})", worst)
    assert worst <= 1


def test_zz_measured():
    """(prints) the largest need_C = |err| / (u (|scale| (S_abs + |bias|) + |resid|)) the kernels above showed"""
    print(f"need_C: convs {NEED['conv']:.2f} (C_TOL_CONV {R.C_TOL_CONV}), VALU ops {NEED['valu']:.2f} "
          f"(C_TOL_VALU {R.C_TOL_VALU})")
