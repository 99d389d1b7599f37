"""float64 references of the vocoder's operations, written from each operation's definition (not from the kernels'
tiling, phase decomposition or summation order), and the tolerance model that compares a kernel's output with them.

Inputs are the exact values a kernel receives (activations and weights already rounded to f16, held as float64), so
the only legitimate differences are the order of the f32 sums, the hardware sine and the f16 rounding of outputs.
Every reference of a weighted sum also returns S_abs = sum |w| |x| per output element: the scale of its f32
summation error.

Tolerances (u = 2^-24; C_tol is measured, see tests/test_gpu_voc_ops.py):
  f32 output v = (sum w x + bias) * scale + resid:
      |gpu - ref| <= C_tol u (|scale| (S_abs + |bias|) + |resid|) + 8 u |ref|              (lin_tol)
      unchanged after an activation of slope <= 1 (tanh, ReLU); after GELU (slope <= 1.13, f16 in and out):
      1.13 (dv + half-ulp_f16(v)) + half-ulp_f16(gelu), against the GELU without its two roundings     (act_tol)
  f16 output f16(snake(v)) with dv the bound of v:
      |gpu - snake64(v_ref)| <= (1 + a ib) dv + 4e-6 ib + 2^-11 (|snake64(v_ref)| + dv) + 2^-25        (f16_tol)
"""
import numpy as np

U = 2.0 ** -24
GELU_C = 0.79788456080286535587989211986876


def f16(x):
    """round to f16, as float64 (numpy converts float64 -> float16 with one rounding)"""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def half_ulp16(x):
    """half the f16 spacing at |x| (2^-25 below the smallest normal)"""
    a = np.minimum(np.abs(np.asarray(x, np.float64)), 65504.0).astype(np.float16)
    return 0.5 * np.spacing(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------ elementwise
def snake(z, a, ib):
    """SnakeBeta z + exp(-beta) sin^2(exp(alpha) z); a = exp(alpha), ib = exp(-beta) per channel (last axis)"""
    z = np.asarray(z, np.float64)
    return z + ib * np.sin(a * z) ** 2


def gelu_smooth(x):
    """ggml's tanh-form GELU with its x <= -10 / x >= 10 branches, without the f16 roundings"""
    x = np.asarray(x, np.float64)
    g = 0.5 * x * (1.0 + np.tanh(GELU_C * x * (1.0 + 0.044715 * x * x)))
    return np.where(x <= -10.0, 0.0, np.where(x >= 10.0, x, g))


def gelu_ggml(x):
    """gelu_ggml of q3t_common.h: the tanh form on the f16-rounded input, the result rounded to f16"""
    x = np.asarray(x, np.float64)
    v = f16(x)
    g = f16(0.5 * v * (1.0 + np.tanh(GELU_C * v * (1.0 + 0.044715 * v * v))))
    return np.where(x <= -10.0, 0.0, np.where(x >= 10.0, x, g))


def act_apply(v, act):
    """conv epilogue activations: 1 tanh, 2 ReLU, 3 tanh(ReLU), 4 GELU (smooth form: see act_tol)"""
    if act == 1:
        return np.tanh(v)
    if act == 2:
        return np.maximum(v, 0.0)
    if act == 3:
        return np.tanh(np.maximum(v, 0.0))
    if act == 4:
        return gelu_smooth(v)
    return v


# ------------------------------------------------------------------------------------------------ convolutions
def causal_conv(x, w, pad, dil, M=None, rows=None):
    """x [T][C_in], w [k][C_out][C_in]; left-pad `pad` zero rows, then y[m] = sum_j W_j x[m + j dil] (rows past the
    end of x read as zero too).  Returns (y, S_abs) for output rows `rows` (default: all M = T + pad - dil (k-1))."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    T, k = x.shape[0], w.shape[0]
    if M is None:
        M = T + pad - dil * (k - 1)
    rows = np.arange(M) if rows is None else np.asarray(rows, np.int64)
    tail = max(0, M + (k - 1) * dil - (T + pad))
    xp = np.concatenate([np.zeros((pad, x.shape[1])), x, np.zeros((tail, x.shape[1]))], 0)
    y = np.zeros((len(rows), w.shape[1]))
    s = np.zeros_like(y)
    for j in range(k):
        xj = xp[rows + j * dil]
        y += xj @ w[j].T
        s += np.abs(xj) @ np.abs(w[j]).T
    return y, s


def transposed_conv(x, w, st, trim, rows=None):
    """scatter form: full[st t + k] += W_k x[t] over (T-1) st + K rows, then `trim` rows cut from both ends.
    x [T][C_in], w [K][C_out][C_in].  Returns (y, S_abs) for the distinct output rows `rows` (default: all)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    T, K = x.shape[0], w.shape[0]
    T_full = (T - 1) * st + K
    T_out = T_full - 2 * trim
    rows = np.arange(max(T_out, 0)) if rows is None else np.asarray(rows, np.int64)
    slot = np.full(T_full, -1, np.int64)     # position of each wanted row of `full` in the output
    slot[rows + trim] = np.arange(len(rows))
    y = np.zeros((len(rows), w.shape[1]))
    s = np.zeros_like(y)
    t = np.arange(T)
    for k in range(K):
        dst = slot[st * t + k]               # x[t] scatters through tap k to full[st t + k]: distinct rows per k
        hit = dst >= 0
        y[dst[hit]] += x[hit] @ w[k].T
        s[dst[hit]] += np.abs(x[hit]) @ np.abs(w[k]).T
    return y, s


def transposed_conv_gather(x, w, st, trim):
    """the per-phase gather form of the same operation (the check of transposed_conv): output row o = st m + phi takes
    taps k = (phi + trim) % st + j st from input row m + (phi + trim - k) / st"""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    T, K = x.shape[0], w.shape[0]
    T_out = (T - 1) * st + K - 2 * trim
    y = np.zeros((max(T_out, 0), w.shape[1]))
    for o in range(T_out):
        m, phi = divmod(o, st)
        for k in range((phi + trim) % st, K, st):
            i = m + (phi + trim - k) // st
            if 0 <= i < T:
                y[o] += w[k] @ x[i]
    return y


def dwconv(x, w, b):
    """depthwise causal conv: y[t][c] = b[c] + sum_j w[c][j] f16(x[t + j - (K-1)][c]); x [T][C], w [C][K]"""
    xq = f16(x)
    T, C = xq.shape
    K = w.shape[1]
    xp = np.concatenate([np.zeros((K - 1, C)), xq], 0)
    y = np.zeros((T, C))
    s = np.zeros((T, C))
    for j in range(K):
        y += xp[j:j + T] * w[:, j]
        s += np.abs(xp[j:j + T] * w[:, j])
    return y + b, s


def conv_out1(xh, w, bias):
    """single-channel output conv: y[t] = tanh(bias + sum_j sum_c w[j][c] xh[t + j - (K-1)][c]); returns the
    pre-activation value too: (y, v, S_abs)"""
    v, s = causal_conv(xh, np.asarray(w, np.float64)[:, None, :], w.shape[0] - 1, 1)
    v = v[:, 0] + bias
    return np.tanh(v), v, s[:, 0]


def f16_round_dev(s, ds):
    """h = f16(s), and how far an evaluation of s with error up to ds may land from h after ITS rounding: one f16
    step where s lies within ds of the boundary between h and a neighbour, else 0.  Returns (h, dh)."""
    s = np.asarray(s, np.float64)
    h16 = s.astype(np.float16)
    h = h16.astype(np.float64)
    lo = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
    hi = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
    near = np.minimum(s - 0.5 * (lo + h), 0.5 * (h + hi) - s) <= ds
    return h, np.where(near, np.maximum(h - lo, hi - h), 0.0)


def resunit(xh, x, w1, b1, a2, ib2, w2, b2, an, ibn, dil, c_tol):
    """h = f16(snake2(conv7_dil(xh) + b1)); x' = x + conv1(h) + b2; y16 = snake_next(x') (unrounded).
    Returns (x', y16, dx): dx the bound of x'.  h is rounded to f16 inside the unit, so an f32 evaluation whose
    snake2 value lies within its own error ds of a rounding boundary may round to the other neighbour: those (and
    only those) elements of h may differ, by one f16 step, and conv1 carries that into x' with |w2|."""
    v1, s1 = causal_conv(xh, w1, 6 * dil, dil)
    ds = (1.0 + a2 * ib2) * lin_tol(c_tol, s1, v1 + b1, bias=b1) + 4e-6 * ib2
    h, dh = f16_round_dev(snake(v1 + b1, a2, ib2), ds)
    w2 = np.asarray(w2, np.float64)
    v2, s2 = causal_conv(h, w2[None], 0, 1)
    xo = x + (v2 + b2)
    dx = lin_tol(c_tol, s2, xo, bias=b2, resid=x) + dh @ np.abs(w2).T
    return xo, snake(xo, an, ibn), dx


# ------------------------------------------------------------------------------------------------ norms, attention
def norm_rows(x, w, b, eps, mode):
    """mode 0 RMSNorm x / sqrt(mean(x^2) + eps) * w; mode 1 LayerNorm (x - mean) / sqrt(var + eps) * w + b.
    Returns (y, mag, mm): mag = |scaled term| + |b| (= |y| where the two do not cancel), the magnitudes the f32
    result's roundings scale with; mm = |mean w / sqrt(var + eps)|, what one rounding of the mean to f32 (the
    operation's own: the mean is an f32 value subtracted from f32 inputs) moves the result by, in units of u."""
    x = np.asarray(x, np.float64)
    if mode == 0:
        t = x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w
        return t, np.abs(t), np.zeros_like(t)
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    rw = w / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    return d * rw + b, np.abs(d * rw) + np.abs(b), np.abs(mean * rw)


def rope_neox(x, rope):
    """x [F][nH][64], rope [F][64] as (cos, sin) pairs: pairs (i, i + 32) rotated by angle i of the row's position"""
    c, s = rope[:, None, 0::2], rope[:, None, 1::2]
    x0, x1 = x[..., :32], x[..., 32:]
    return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], -1)


def attention(q, k, v):
    """causal softmax attention, scale 1/8; q, k, v [F][nH][64] (RoPE applied).  Returns (out, allow): allow =
    (1 + 2 max_k sum_d |q_d k_d| / 8) max_k |v_kd| per output element, the scale of the f32 evaluation's error"""
    F = q.shape[0]
    sc = np.einsum("qhd,khd->hqk", q, k) / 8.0
    sa = np.einsum("qhd,khd->hqk", np.abs(q), np.abs(k)) / 8.0
    mask = np.tril(np.ones((F, F), bool))
    sc = np.where(mask, sc, -np.inf)
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    out = np.einsum("hqk,khd->qhd", p, v)
    smax = np.where(mask, sa, 0.0).max(-1)                                  # [h][q]
    vmax = np.maximum.accumulate(np.abs(v), axis=0)                         # [q][h][d]: max over keys <= q
    return out, (1.0 + 2.0 * smax.T)[:, :, None] * vmax


# ------------------------------------------------------------------------------------------------ tolerance model
# C_tol: 4 x the larger of the float32 re-evaluation's worst |err| / (u S_abs) on the CPU (tests/test_voc_ops_ref.py)
# and the kernels' own on their first green run; the measured figures are in the header of tests/test_gpu_voc_ops.py
C_TOL_CONV = 10.4   # the MFMA convs (k_conv, k_conv_mt, k_conv_pd, k_resunit96): 4 x max(1.75 CPU, 2.59 GPU)
C_TOL_VALU = 12.7   # the VALU ops (k_conv_out1, k_dwconv, k_attn_prefill): 4 x max(2.83 CPU, 3.17 GPU)


def lin_tol(c_tol, s_abs, ref, bias=0.0, scale=1.0, resid=0.0):
    return c_tol * U * (np.abs(scale) * (s_abs + np.abs(bias)) + np.abs(resid)) + 8 * U * np.abs(ref)


def act_tol(dv, v_ref, act):
    """the bound of act(v) given the bound dv of v (compared with act_apply(v_ref, act))"""
    if act == 4:
        return 1.13 * (dv + half_ulp16(v_ref)) + half_ulp16(gelu_smooth(v_ref))
    return dv


def f16_tol(dv, s_ref, a=0.0, ib=0.0):
    """the bound of f16(snake(v)) compared with s_ref = snake64(v_ref) (a = ib = 0: plain rounding)"""
    return (1.0 + a * ib) * dv + 4e-6 * ib + 2.0 ** -11 * (np.abs(s_ref) + dv) + 2.0 ** -25


def norm_tol(ref, mag, mm):
    """the norms sum in double: 16 u on the magnitudes of the result's terms, one rounding of the mean, f16 rounding"""
    return f16_tol(16 * U * mag + U * mm, ref)


def attn_tol(c_tol, ref, allow):
    return f16_tol(c_tol * U * allow, ref)


def need_c(got, ref, unit, fixed=0.0):
    """the C_tol an output would need: max (|got - ref| - fixed) / unit"""
    return float(np.max((np.abs(np.asarray(got, np.float64) - ref) - fixed) / unit)) if np.size(ref) else 0.0


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over every element (inf where an element is not finite)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(got), err, np.inf)
    return float(np.max(err / tol)) if err.size else 0.0
