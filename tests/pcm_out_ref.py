"""numpy-only float64 restatement of the output stage (csrc/pcm_out.h, DESIGN 2c "Output stage"): the polyphase filter
design, the run over a whole signal, a chunked run with a carried history, s16 and G.711 mu-law.  No scipy.

Every function takes the wrong variants of tests/test_pcm_out_ref.py as keyword switches (all off by default), so that
the mutation checks exercise the same code the comparisons use."""
import math

import numpy as np

RATES = (8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
NATIVE = 24000
Z = 16
BETA = 9.0
F32, S16, MULAW = 0, 1, 2
DTYPES = {F32: np.float32, S16: np.int16, MULAW: np.uint8}


def geometry(rate):
    """(L, M, K, D): up, down, taps per phase, zero samples a final push appends.  24000 is the bypass: K = 0, D = 0"""
    if rate not in RATES:
        raise ValueError(f"unsupported rate {rate}")
    if rate == NATIVE:
        return 1, 1, 0, 0
    g = math.gcd(rate, NATIVE)
    L, M = rate // g, NATIVE // g
    R = max(L, M)
    N = 2 * Z * R + 1
    return L, M, -(-N // L), -(-(Z * R) // L)


def i0(x):
    """modified Bessel function of the first kind, order 0, by its power series (float64, elementwise)"""
    x = np.asarray(x, np.float64)
    q = x * x / 4.0
    term = np.ones_like(q)
    total = np.ones_like(q)
    for k in range(1, 500):
        term = term * q / (k * k)
        total = total + term
        if np.all(term < total * 1e-18):
            break
    return total


def prototype(rate):
    """h[0 .. N) in float64: f * sinc(f * (j - c)) * kaiser(beta 9)"""
    L, M, _, _ = geometry(rate)
    R = max(L, M)
    N, c, f = 2 * Z * R + 1, Z * R, 0.9 / R
    u = np.arange(N, dtype=np.float64) - c
    w = i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (u / c) ** 2))) / i0(BETA)
    return f * np.sinc(f * u) * w     # np.sinc(x) = sin(pi x) / (pi x)


def taps64(rate):
    """taps[p][k] = L * h[p + k * L] in float64, 0 where p + k * L >= N; shape [L][K]"""
    L, M, K, _ = geometry(rate)
    if K == 0:
        return np.zeros((1, 0), np.float64)
    h = prototype(rate)
    t = np.zeros((L, K), np.float64)
    for p in range(L):
        hp = h[p::L]
        t[p, :len(hp)] = L * hp
    return t


def taps32(rate):
    return taps64(rate).astype(np.float32)


def num_samples(n_in_total, rate, final=False):
    L, M, _, D = geometry(rate)
    S = int(n_in_total) + (D if final else 0)
    return -(-(S * L) // M)


def _fir(xpad, pad, n_idx, L, M, K, taps, dtype, phase_off=0, drop_tap=None):
    """y[n] for the global output indices n_idx over xpad, whose element j is global input sample j - pad.
    Returns (y, bound) with bound[n] = sum_k |taps * x|.  dtype float64: the reference; float32: the kernel's loop"""
    t = n_idx.astype(np.int64) * M + phase_off
    i, p = t // L, t % L
    tp = np.asarray(taps)[p]                                     # [n][K]
    if drop_tap is not None:
        tp = tp.copy()
        tp[:, drop_tap] = 0
    win = xpad[(i[:, None] + pad - np.arange(K)[None, :])]       # x[i - k]
    if dtype == np.float32:
        # the pinned chain: acc = fmaf(tap, x, acc) from 0.0f, k upward.  One rounding per step: the product and the
        # sum are formed in float64 (exact for f32 operands up to the final rounding of the sum) and rounded once
        acc = np.zeros(len(n_idx), np.float32)
        for k in range(K):
            acc = (tp[:, k].astype(np.float64) * win[:, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        y = acc
    else:
        y = (tp.astype(np.float64) * win.astype(np.float64)).sum(axis=1)
    bound = np.abs(tp.astype(np.float64) * win.astype(np.float64)).sum(axis=1)
    return y, bound


def resample(x, rate, final=True, taps=None, dtype=np.float64, with_bound=False, **mut):
    """the whole signal x (the vocoder's samples from the start of the stream) at `rate`; taps default to taps32"""
    x = np.asarray(x)
    L, M, K, D = geometry(rate)
    n_out = num_samples(len(x), rate, final)
    if K == 0:
        y = x.astype(dtype)
        return (y, np.abs(y).astype(np.float64)) if with_bound else y
    taps = taps32(rate) if taps is None else taps
    xpad = np.concatenate([np.zeros(K - 1, x.dtype), x, np.zeros(D + 1, x.dtype)])
    y, b = _fir(xpad, K - 1, np.arange(n_out), L, M, K, taps, dtype, **mut)
    return (y, b) if with_bound else y


class RefStream:
    """the chunked run: push(x, final) returns the outputs the stream owes after these samples, from a carried history
    of the last K - 1 input samples and the two running counts -- the host-side bookkeeping restated"""

    def __init__(self, rate, taps=None, dtype=np.float64, hist_short=0):
        self.rate = rate
        self.L, self.M, self.K, self.D = geometry(rate)
        self.taps = taps32(rate) if taps is None and self.K else taps
        self.dtype = dtype
        self.hist_short = hist_short          # mutation: the history holds this many samples fewer
        self.hist = np.zeros(max(self.K - 1, 0), np.float64)
        self.s0 = 0                           # input samples consumed
        self.n0 = 0                           # outputs produced
        self.final = False

    def push(self, x, final=False):
        assert not self.final, "push after final"
        x = np.asarray(x, np.float64)
        total = num_samples(self.s0 + len(x), self.rate, final)
        n_idx = np.arange(self.n0, total)
        if self.K == 0:
            y = x.astype(self.dtype)
        else:
            hist = self.hist.copy()
            if self.hist_short:
                hist[:self.hist_short] = 0.0
            xpad = np.concatenate([hist, x, np.zeros(self.D + 1)])
            # element j of xpad is global sample s0 - (K - 1) + j
            y, self.last_bound = _fir(xpad, self.K - 1 - self.s0, n_idx, self.L, self.M, self.K, self.taps, self.dtype)
            allx = np.concatenate([self.hist, x, np.zeros(self.D if final else 0)])
            self.hist = allx[len(allx) - (self.K - 1):]
        self.s0 += len(x)
        self.n0 = total
        self.final = bool(final)
        return y


def to_s16(y, rounding=False):
    """(int16)(clamp(y, -1, 1) * 32767.0f), truncated toward zero, in float32 (save_audio_file's rule)"""
    c = np.clip(np.asarray(y, np.float32), np.float32(-1), np.float32(1)) * np.float32(32767)
    if rounding:
        c = np.rint(c)
    return c.astype(np.int16)


def mulaw_encode(s16):
    """G.711 mu-law of int16 values: bias 0x84, clip 32635, sign / exponent / mantissa complemented"""
    v = np.asarray(s16).astype(np.int32)
    sign = np.where(v < 0, 0x80, 0)
    m = np.minimum(np.abs(v), 32635) + 132
    e = np.frexp(m.astype(np.float64))[1].astype(np.int32) - 8   # top set bit 7 .. 14 -> 0 .. 7
    mant = (m >> (e + 3)) & 0xF
    return (~(sign | (e << 4) | mant) & 0xFF).astype(np.uint8)


def mulaw_decode(u8):
    """the G.711 expansion (for the monotonicity check): uint8 -> int32 linear value"""
    u = ~np.asarray(u8).astype(np.int32) & 0xFF
    sign, e, mant = u & 0x80, (u >> 4) & 7, u & 0xF
    mag = (((mant << 3) + 132) << e) - 132
    return np.where(sign != 0, -mag, mag)


def convert(y32, fmt):
    """the kernel's output of format fmt from its f32 samples"""
    if fmt == F32:
        return np.asarray(y32, np.float32)
    s = to_s16(y32)
    return s if fmt == S16 else mulaw_encode(s)


def gamma(K):
    """the fma chain's bound factor: K * 2^-24 / (1 - K * 2^-24)"""
    u = K * 2.0 ** -24
    return u / (1.0 - u)
