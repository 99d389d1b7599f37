"""float64 reference and tolerance of the vocoder stream's attention over its K/V cache (k_voc_kv_append,
k_voc_attn_cached; tests/test_gpu_voc_stream_ops.py), in the style of tests/voc_ops_ref.py.

The n queries sit at absolute positions P .. P+n-1 and attend to cache rows 0 .. their own position.  The tolerance
has voc_ops_ref.attn_tol's form, f16_tol(C u allow, ref) with allow = (1 + 2 max_k sum_d |q_d k_d| / 8) max_k |v_kd|;
its constant C_TOL_STREAM is 4 x the worst need of eval32, a float32 re-evaluation of the reference in the kernel's
summation structure (sequential dot products, 64-key chunks from key 0, online softmax, key-by-key P.V), measured on
the CPU over the GPU test's own cases by tests/test_voc_stream_ops_ref.py -- never taken from the kernel under test.
"""
import numpy as np

import voc_ops_ref as R

U = R.U
CASES = ((0, 1), (0, 33), (63, 1), (64, 1), (63, 2), (100, 70))   # (P, n)
HEADS = (2, 16)
# 4 x the largest float32 re-evaluation need over CASES x HEADS (test_voc_stream_ops_ref.py prints it: 0.395)
C_TOL_STREAM = 1.59


def case(P, n, nH):
    """the inputs of one case: qkv [P+n][3][nH][64] f32 (unrotated), rope [P+n][64] f32 (cos, sin) pairs"""
    rng = np.random.default_rng(1000 * P + 10 * n + nH)
    F = P + n
    qkv = rng.standard_normal((F, 3, nH, 64), dtype=np.float32)
    ang = rng.uniform(0, 2 * np.pi, (F, 32))
    rope = np.stack([np.cos(ang), np.sin(ang)], -1).reshape(F, 64).astype(np.float32)
    return qkv, rope


def rope32(x, rope):
    """k_rope_qk's rotation in float32, each operation rounded (x [F][nH][64] f32, rope [F][64] f32); the kernels may
    contract a product into the sum, so this is a value reference, not a bit reference"""
    c, s = rope[:, None, 0::2], rope[:, None, 1::2]
    x0, x1 = x[..., :32], x[..., 32:]
    return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], -1).astype(np.float32)


def attention_rows(q, K, V, P):
    """q [n][nH][64] at positions P..P+n-1, K / V [P+n][nH][64] (RoPE applied), all float64.  Returns (out, allow)"""
    n, Ft = q.shape[0], K.shape[0]
    sc = np.einsum("qhd,khd->hqk", q, K) / 8.0
    sa = np.einsum("qhd,khd->hqk", np.abs(q), np.abs(K)) / 8.0
    mask = np.arange(Ft)[None, :] <= (P + np.arange(n))[:, None]
    sc = np.where(mask, sc, -np.inf)
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    out = np.einsum("hqk,khd->qhd", p, V)
    smax = np.where(mask, sa, 0.0).max(-1)                       # [h][q]
    vcum = np.maximum.accumulate(np.abs(V), axis=0)              # [k][h][d]: max over keys <= k
    return out, (1.0 + 2.0 * smax.T)[:, :, None] * vcum[P:P + n]


def eval32(q, K, V, P):
    """the same in float32 in k_attn_prefill's structure: per 64-key chunk from key 0 a sequential dot product over d,
    the online-softmax update, then P.V key by key; the result before the f16 rounding"""
    f = np.float32
    q, K, V = q.astype(f), K.astype(f), V.astype(f)
    n, nH = q.shape[0], q.shape[1]
    Ft = K.shape[0]
    qpos = P + np.arange(n)
    m = np.full((n, nH), -np.inf, f)
    l = np.zeros((n, nH), f)
    acc = np.zeros((n, nH, 64), f)
    with np.errstate(invalid="ignore"):
        for k0 in range(0, Ft, 64):
            Kc, Vc = K[k0:k0 + 64], V[k0:k0 + 64]
            kc = Kc.shape[0]
            live = qpos >= k0                                         # queries whose tile reaches this chunk
            if not live.any():
                break
            ds = np.zeros((n, nH, kc), f)
            for d in range(64):
                ds = ds + q[:, :, None, d] * Kc.transpose(1, 0, 2)[None, :, :, d]
            ok = (k0 + np.arange(kc))[None, :] <= qpos[:, None]       # [n][kc]
            sc = np.where(ok[:, None, :], ds * f(0.125), f(-np.inf))
            mn = np.maximum(m, sc.max(-1))
            corr = np.where(np.isinf(m), f(0), np.exp(m - mn)).astype(f)
            pv = np.where(np.isinf(sc), f(0), np.exp(sc - mn[:, :, None])).astype(f)
            ls = np.zeros((n, nH), f)
            for kk in range(kc):
                ls = ls + pv[:, :, kk]
            upd = live[:, None]
            l = np.where(upd, l * corr + ls, l)
            acc_n = acc * corr[:, :, None]
            for kk in range(kc):
                acc_n = acc_n + pv[:, :, kk, None] * Vc[kk][None, :, :]
            acc = np.where(upd[:, :, None], acc_n, acc)
            m = np.where(upd, mn, m)
    return acc * (f(1.0) / l)[:, :, None]


def tol(ref, allow):
    return R.f16_tol(C_TOL_STREAM * U * allow, ref)
