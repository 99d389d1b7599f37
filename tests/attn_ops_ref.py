"""float64 references of the decode and prefill attention kernels (csrc/attn.hip, attn_seq.h, attn_small.h), written
from the operation's definition, the input generator that leaves the kernels' on-chip f16 roundings no ambiguity, the
float32 re-evaluations that define the tolerance constant, and the tolerance itself.

The operation, per slot (src semantics: Qwen3 block): the R = nH / nKV q heads of kv head g and the new k row get the
head RMSNorm x / sqrt(mean(x^2) + eps) * w and NEOX RoPE at the slot's position, rounded to f16 (q^, k^); the new v row
is the f16 rounding of the raw one (v^).  k^ and v^ become cache row pos.  Scores are q^ . K_j / sqrt(D) over rows
j <= pos (row pos the new one), the output sum_j p_j V_j / sum_j p_j with p_j = exp(s_j - max s), rounded to f16.
The prefill is the same for row i of an utterance over its own rows 0..i.

Inputs without rounding ambiguity: a float32 prologue may land on the other side of an f16 rounding boundary from the
float64 one, so every q / k head vector is drawn by rejection (seeded) until no element of prologue64 lies within
MARGIN u (|a c| + |b s|) of an f16 rounding boundary (u = 2^-24, |a c| + |b s| the magnitude of the element's two RoPE
terms).  A float32 replica of the kernels' prologue (prologue32) differs from float64 by at most 4.5 u of that magnitude
(tests/test_attn_ops_ref.py::test_generator_rounds_alike prints it: 4.10 over 4,002 accepted vectors at scales 1e-3, 1,
1e3, D 64 and 128; 4.48 over the set a margin of 17.2 accepted).  MARGIN = 4 x 4.5 = 18; about one plain draw in two to
three is accepted.  With such inputs the appended K / V rows equal the reference bit for bit and q^ is the same on both
sides.

Tolerance of an output element: voc_ops_ref.f16_tol(C_TOL_ATTN u allow + exp_term, ref) with
  allow = (sum_j p_j |V_jd| / sum_j p_j) (1 + max_j sum_d |q^_d K_jd| / sqrt(D) + max_j |s_j - m|)
          (the accumulation's magnitude times the relative error of a weight: the score's own rounding error and the
          exponent's argument)
  exp_term, only where the kernel exponentiates with __expf (v_exp_f32, 1 ulp = 2 u relative, on x log2(e) rounded to
          f32, ~1.45 |x| u): a weight that is the product of n_exp such exponentials whose arguments sum to
          x_j = s_j - m carries (2 n_exp + 1.45 |x_j|) u, so
          exp_term = u (2 n_exp (A_d + |ref_d|) + 1.45 (sum_j p_j |x_j| |V_jd| / sum_j p_j + |ref_d| sum_j p_j |x_j| / sum_j p_j))
          with A_d = sum_j p_j |V_jd| / sum_j p_j.  n_exp = 1 for k_attn and k_prefill_attn (their combine uses expf),
          1 + the number of 64-position chunks for k_attn_seq (one rescale per chunk), 0 for k_attn_small (expf).
  C_TOL_ATTN = 4 x the largest need of a float32 re-evaluation of the reference on the CPU, need = |f32 - f64| /
          (u allow), in the four summation structures the kernels use (eval32): measured by
          tests/test_attn_ops_ref.py::test_f32_reevaluations (printed there):
              sequential 0.65, pairwise tree 0.51, per-wave online softmax with chunk rescale and 4-way merge 0.47,
              split partials with exponent-weighted combine 0.58       => C_TOL_ATTN = 4 x 0.654 = 2.62
  The kernels on an MI355X (tests/test_gpu_attn_ops.py prints each test's need; for information, never copied into
  the constant).  An f16 output shows of the f32 value behind it only what leaves its own rounding interval
  (need()), so these are lower bounds, after / before exp_term is taken off:
      k_attn 0.00 / 0.13, k_attn_seq 0.00 / 0.08, k_attn_small 0.22 / 0.22 (no exp_term), k_prefill_attn 0.10 / 0.28
  all below the CPU's own 0.65; the outputs' worst |err| / tol is 0.99, the f16 half-ulp itself.
"""
import numpy as np

import voc_ops_ref as VR

U = VR.U
MARGIN = 18.0        # rejection margin of the generator, in u (|a c| + |b s|): 4 x 4.5 (measured: docstring)
C_TOL_ATTN = 2.62    # 4 x 0.654 (CPU float32 re-evaluation, see the docstring)
EPS = float(np.float32(1e-6))
POISON = 0x7E01      # f16 NaN


# ------------------------------------------------------------------------------------------------ prologue
def prologue64(raw, w, rope_row, eps, D, interleaved=False):
    """head RMSNorm then NEOX RoPE of raw [..., D] with (cos, sin) = rope_row[..., 2i], rope_row[..., 2i + 1] for
    i < D / 2: element i pairs with i + D / 2.  Returns (y, mag): mag = |a c| + |b s| of each element's two terms.
    interleaved: the wrong pairing (2i, 2i + 1), for the mutation checks."""
    raw = np.asarray(raw, np.float64)
    rope_row = np.asarray(rope_row, np.float64)
    h = D // 2
    t = raw / np.sqrt((raw * raw).mean(-1, keepdims=True) + eps) * np.asarray(w, np.float64)
    c, s = rope_row[..., 0::2], rope_row[..., 1::2]
    a, b = (t[..., 0::2], t[..., 1::2]) if interleaved else (t[..., :h], t[..., h:])
    y0, y1 = a * c - b * s, a * s + b * c
    m0, m1 = np.abs(a * c) + np.abs(b * s), np.abs(a * s) + np.abs(b * c)
    if interleaved:
        y, mag = np.empty_like(t), np.empty_like(t)
        y[..., 0::2], y[..., 1::2], mag[..., 0::2], mag[..., 1::2] = y0, y1, m0, m1
        return y, mag
    return np.concatenate([y0, y1], -1), np.concatenate([m0, m1], -1)


def prologue32(raw, w, rope_row, eps, D):
    """the kernels' prologue in float32 with their roundings: f32 squares summed in double, 1 / sqrtf((float)(ss / D) +
    eps), (x * scale) * w, every RoPE product and sum rounded"""
    x = np.asarray(raw, np.float32)
    w = np.asarray(w, np.float32)
    r = np.asarray(rope_row, np.float32)
    h = D // 2
    ss = (x * x).astype(np.float64).sum(-1, keepdims=True)
    scale = np.float32(1.0) / np.sqrt((ss / D).astype(np.float32) + np.float32(eps))
    t = (x * scale) * w
    c, s = r[..., 0::2], r[..., 1::2]
    a, b = t[..., :h], t[..., h:]
    return np.concatenate([a * c - b * s, a * s + b * c], -1)


def boundary_dist(y):
    """distance of each value to the nearest f16 rounding boundary (the midpoint of two neighbouring f16 values)"""
    y = np.asarray(y, np.float64)
    h16 = y.astype(np.float16)
    h = h16.astype(np.float64)
    lo = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
    hi = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
    return np.minimum(y - 0.5 * (lo + h), 0.5 * (h + hi) - y)


def draw_heads(rng, scale, w, ropes, eps, D):
    """n raw f32 head vectors [n][D] of standard deviation scale[n], each redrawn until prologue64 under every one of
    its RoPE rows ropes[n][C][D] is farther than MARGIN u mag from an f16 rounding boundary in every element"""
    scale = np.asarray(scale, np.float32).reshape(-1)
    ropes = np.asarray(ropes, np.float64)
    n = len(scale)
    raw = np.zeros((n, D), np.float32)
    todo = np.arange(n)
    for _ in range(400):
        if not len(todo):
            return raw
        cand = rng.standard_normal((len(todo), D), dtype=np.float32) * scale[todo, None]
        y, mag = prologue64(cand[:, None, :], w, ropes[todo], eps, D)
        ok = (boundary_dist(y) > MARGIN * U * mag).all((1, 2))
        raw[todo[ok]] = cand[ok]
        todo = todo[~ok]
    raise AssertionError("draw_heads: no acceptable vector in 400 draws")


def rope_table(n_rows, D, theta=10000.0):
    """[n_rows][D] f32 (cos, sin) pairs of angle pos * theta^(-2i / D)"""
    i = np.arange(D // 2)
    ang = np.arange(n_rows)[:, None] * theta ** (-2.0 * i / D)[None]
    return np.stack([np.cos(ang), np.sin(ang)], -1).reshape(n_rows, D).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the reference
def _attend64(qh, K, V, D, mut):
    """one q head over rows K, V [n][D] (the last the new one).  mut: see decode64"""
    n = K.shape[0]
    kq = 1.0 if mut.get("no_scale") else 1.0 / np.sqrt(D)
    s = K @ qh * kq
    sabs = np.abs(K) @ np.abs(qh) / np.sqrt(D)
    live = np.ones(n, bool)
    for j in mut.get("drop", ()):
        if 0 <= j < n:
            live[j] = False
    if "split_drop" in mut:
        ch, sp = mut["split_drop"]
        live[sp * ch:(sp + 1) * ch] = False
    m = s[live].max()
    x = s - m
    p = np.where(live, np.exp(x), 0.0)
    if "split_w1" in mut:       # that split's partial, relative to its own maximum, combined with weight 1
        ch, sp = mut["split_w1"]
        sl = slice(sp * ch, min((sp + 1) * ch, n))
        p[sl] = np.exp(s[sl] - s[sl].max())
    l = p.sum()
    out = p @ V / l
    A = p @ np.abs(V) / l
    return dict(out=out, allow=A * (1.0 + sabs[live].max() + np.abs(x[live]).max()), A=A,
                px=(p * np.abs(x)) @ np.abs(V) / l, px1=float((p * np.abs(x)).sum() / l))


def decode64(qkv, qn, kn, rope_row, eps, kc, vc, pos, nH, nKV, D, mut=None):
    """one slot.  qkv: the raw row [(nH + 2 nKV) D]; kc, vc [nKV][>= pos rows][D]: the cache's f16 values (rows < pos
    are read; row pos too under the `stale` mutation).  Returns a dict: out [nH][D] (unrounded), k_new / v_new
    [nKV][D] (the f16 values of cache row pos), allow, A, px [nH][D], px1 [nH] (the tolerance's terms, tol()).
    mut (mutation checks only; applied to the reference): drop = positions left out, split_drop = (chunk, split) left
    out of the combine, split_w1 = (chunk, split) combined with weight 1, stale = row pos read from the cache, kvmap =
    "mod" (q head h -> kv head h % nKV), interleaved, no_scale; `operands` = a list that receives (q^, K, V) per head"""
    mut = mut or {}
    qkv = np.asarray(qkv, np.float64).reshape(nH + 2 * nKV, D)
    R = nH // nKV
    q_hat = VR.f16(prologue64(qkv[:nH], qn, rope_row, eps, D, mut.get("interleaved", False))[0])
    k_new = VR.f16(prologue64(qkv[nH:nH + nKV], kn, rope_row, eps, D, mut.get("interleaved", False))[0])
    v_new = VR.f16(qkv[nH + nKV:])
    res = dict(out=np.zeros((nH, D)), allow=np.zeros((nH, D)), A=np.zeros((nH, D)), px=np.zeros((nH, D)),
               px1=np.zeros(nH), k_new=k_new, v_new=v_new)
    for h in range(nH):
        g = h % nKV if mut.get("kvmap") == "mod" else h // R
        if mut.get("stale"):
            K, V = kc[g][:pos + 1], vc[g][:pos + 1]
        else:
            K = np.concatenate([kc[g][:pos], k_new[g][None]], 0)
            V = np.concatenate([vc[g][:pos], v_new[g][None]], 0)
        if "operands" in mut:
            mut["operands"].append((q_hat[h], K, V))
        r = _attend64(q_hat[h], K, V, D, mut)
        for k in ("out", "allow", "A", "px"):
            res[k][h] = r[k]
        res["px1"][h] = r["px1"]
    return res


def prefill64(qkv, qn, kn, rope, eps, nH, nKV, D, mut=None):
    """one utterance: qkv [plen][(nH + 2 nKV) D]; row i is decode64 at position i over the utterance's own rows 0..i.
    Returns the dict of decode64 with a leading row axis (k_new / v_new: the cache rows 0..plen-1 [plen][nKV][D])"""
    plen = qkv.shape[0]
    kc, vc = np.zeros((nKV, plen, D)), np.zeros((nKV, plen, D))
    rows = []
    for i in range(plen):
        r = decode64(qkv[i], qn, kn, rope[i], eps, kc, vc, i, nH, nKV, D, mut)
        kc[:, i], vc[:, i] = r["k_new"], r["v_new"]
        rows.append(r)
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def tab_rows(tab_tok, S, tab_ld, tab_col, tab_row0):
    """k_attn_small's gather: the table row of each slot"""
    return tab_row0 + np.asarray(tab_tok).reshape(-1)[np.arange(S) * tab_ld + tab_col]


# ------------------------------------------------------------------------------------------------ tolerance
def exp_term(res, n_exp):
    """the derived allowance of n_exp __expf factors per weight (docstring); 0 for n_exp = 0"""
    if not n_exp:
        return 0.0
    ref = np.abs(res["out"])
    px1 = np.asarray(res["px1"])[..., None]
    return U * (2.0 * n_exp * (res["A"] + ref) + 1.45 * (res["px"] + ref * px1))


def tol(res, n_exp=0):
    return VR.f16_tol(C_TOL_ATTN * U * res["allow"] + exp_term(res, n_exp), res["out"])


def need(got, res, n_exp=0):
    """what a kernel's f16 output shows of its f32 error, in u allow: (need, raw).  The value before the output's own
    rounding lay within half an f16 step of `got`, so it was at least |got - ref| - half_ulp16(got) from the reference
    (0 where the reference lies inside that interval: most elements).  raw is the largest such distance; need the
    largest after exp_term is taken off, the figure to hold against C_TOL_ATTN."""
    got = np.asarray(got, np.float64)
    least = np.maximum(np.abs(got - res["out"]) - VR.half_ulp16(got), 0.0)
    unit = U * res["allow"]
    return (float(np.max(np.maximum(least - exp_term(res, n_exp), 0.0) / unit)), float(np.max(least / unit)))


# ------------------------------------------------------------------------------------------------ float32 re-evaluations
F32 = np.float32


def _seq(a, axis=0):
    return np.cumsum(a, axis=axis, dtype=F32).take(-1, axis)


def _tree(a):
    """pairwise tree over axis 0 (neighbours, then pairs of pairs ...), zero-padded to a power of two"""
    a = np.asarray(a, F32)
    n = 1
    while n < a.shape[0]:
        n *= 2
    a = np.concatenate([a, np.zeros((n - a.shape[0],) + a.shape[1:], F32)], 0)
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def _scores32(q, K, D, tree):
    prod = (K.astype(F32) * q.astype(F32)[None]).T            # exact: f16 x f16
    return (_tree(prod) if tree else _seq(prod)) * (F32(1.0) / np.sqrt(F32(D)))


def _part32(s, V, summ):
    """(m, l, acc) of one group of positions: its own maximum, f32 exponentials"""
    m = s.max()
    p = np.exp(s - m)
    return m, summ(p), summ(p[:, None] * V.astype(F32))


def eval32(structure, q, K, V, D, chunk=64):
    """the reference re-evaluated in float32 in one of the kernels' summation structures.  q [D], K, V [n][D] (f16
    values).  sequential: k_attn_small; tree: k_prefill_attn and the inside of a k_attn chunk; online: k_attn_seq
    (four waves, each over its 16 positions of every 64-chunk with a rescale per chunk, merged at the end); split:
    k_attn (one partial per chunk, tree inside, combined with exp(m_s - m) in order)"""
    n = K.shape[0]
    if structure in ("sequential", "tree"):
        tree = structure == "tree"
        m, l, acc = _part32(_scores32(q, K, D, tree), V, _tree if tree else _seq)
        return acc / l
    if structure == "split":
        s = _scores32(q, K, D, True)
        parts = [_part32(s[j:j + chunk], V[j:j + chunk], _tree) for j in range(0, n, chunk)]
        if len(parts) == 1:
            return parts[0][2] / parts[0][1]
        mx = max(p[0] for p in parts)
        l, acc = F32(0), np.zeros(D, F32)
        for m, ls, a in parts:
            w = np.exp(F32(m - mx))
            l = F32(ls * w + l)
            acc = a * w + acc
        return acc / l
    assert structure == "online"
    s = _scores32(q, K, D, True)
    j = np.arange(n)
    wave = (j % 16) // 4
    st = []
    for w in range(4):
        m, l, acc = F32(-np.inf), F32(0), np.zeros(D, F32)
        for c in range(0, n, 64):
            sel = (wave == w) & (j >= c) & (j < c + 64)
            if not sel.any():
                continue
            mn = max(m, s[sel].max())
            alpha = np.exp(F32(m - mn))
            p = np.exp(s[sel] - mn)
            l = F32(l * alpha) + _seq(p)
            acc = acc * alpha
            for pj, vj in zip(p, V[sel].astype(F32)):
                acc = pj * vj + acc
            m = mn
        st.append((m, l, acc))
    M = max(x[0] for x in st)
    num, den = np.zeros(D, F32), F32(0)
    for m, l, acc in st:
        if m == -np.inf:
            continue
        f = np.exp(F32(m - M))
        num, den = acc * f + num, F32(l * f + den)
    return num / den


# ------------------------------------------------------------------------------------------------ cases
def h16bits(a):
    """float64 values that are exact f16 -> their bits"""
    return np.asarray(a).astype(np.float16).view(np.uint16)


def decode_case(seed, D, R, nKV, n_ctx, poss, scales, peaked=False, k_sd=0.5, tab=None):
    """the inputs of one attn_decode launch, one slot per entry of poss (raw standard deviation scales[slot]): head-norm
    weights exp(0.3 N) (qn x 6 when peaked), the RoPE table, cache rows < pos random f16 (K of standard deviation
    k_sd), rows >= pos -- row pos included -- f16 NaN poison, and the raw QKV rows with their q / k head vectors drawn
    by draw_heads.  tab = dict(rows, ld, col, row0, tok): the rows come from a per-token table instead (k_attn_small's
    qkv_tab: slot s reads table row row0 + tok[s]; slots sharing a token share the row, accepted at both positions)"""
    rng = np.random.default_rng(seed)
    S, nH = len(poss), R * nKV
    poss = np.asarray(poss, np.int32)
    qn = np.exp(0.3 * rng.standard_normal(D)).astype(np.float32) * np.float32(6.0 if peaked else 1.0)
    kn = np.exp(0.3 * rng.standard_normal(D)).astype(np.float32)
    rope = rope_table(int(poss.max()) + 2, D)
    kc = np.full((S, nKV, n_ctx, D), POISON, np.uint16)
    vc = np.full((S, nKV, n_ctx, D), POISON, np.uint16)
    for s, pos in enumerate(poss):
        kc[s, :, :pos] = h16bits(rng.standard_normal((nKV, pos, D), dtype=np.float32) * np.float32(k_sd))
        vc[s, :, :pos] = h16bits(rng.standard_normal((nKV, pos, D), dtype=np.float32))
    scales = np.asarray(scales, np.float32)
    case = dict(D=D, R=R, nKV=nKV, nH=nH, S=S, n_ctx=n_ctx, pos=poss, qn=qn, kn=kn, rope=rope, kc=kc, vc=vc, eps=EPS)
    if tab is None:
        owner = np.arange(S)                    # the row of each slot
        cond = [[s] for s in range(S)]          # the slots (positions) each row must be accepted at
        nrow = S
    else:
        tok = np.asarray(tab["tok"])
        uniq = sorted(set(int(t) for t in tok))
        owner = np.array([uniq.index(int(t)) for t in tok])
        cond = [[s for s in range(S) if owner[s] == r] for r in range(len(uniq))]
        nrow = len(uniq)
    C = max(len(c) for c in cond)
    rr = np.stack([rope[poss[[c[i % len(c)] for i in range(C)]]] for c in cond])        # [nrow][C][D]
    rsc = np.array([scales[c[0]] for c in cond], np.float32)
    rows = np.zeros((nrow, nH + 2 * nKV, D), np.float32)
    for h in range(nH + nKV):
        rows[:, h] = draw_heads(rng, rsc, qn if h < nH else kn, rr, EPS, D)
    rows[:, nH + nKV:] = rng.standard_normal((nrow, nKV, D), dtype=np.float32) * rsc[:, None, None]
    rows = rows.reshape(nrow, -1)
    case["qkv"] = rows[owner]                   # [S][QKV]: what each slot's launch row holds
    if tab is not None:
        table = rng.standard_normal((tab["rows"], rows.shape[1]), dtype=np.float32)
        tab_tok = rng.integers(0, tab["rows"] - tab["row0"], (S, tab["ld"])).astype(np.int32)
        tab_tok[:, tab["col"]] = tok
        nr = tab["rows"] - tab["row0"]          # the neighbouring columns name other rows (the mutation checks)
        tab_tok[:, tab["col"] - 1], tab_tok[:, tab["col"] + 1] = (tok + 11) % nr, (tok + 17) % nr
        for r, t in enumerate(uniq):
            table[tab["row0"] + t] = rows[r]
        case.update(table=table, tab_tok=tab_tok, tab_ld=tab["ld"], tab_col=tab["col"], tab_row0=tab["row0"])
    return case


def decode_ref(case, s, mut=None, **over):
    """decode64 of slot s of a decode_case (over: replaced arguments, for the mutation checks)"""
    kc = case["kc"][s].view(np.float16).astype(np.float64)
    vc = case["vc"][s].view(np.float16).astype(np.float64)
    a = dict(qkv=case["qkv"][s], qn=case["qn"], kn=case["kn"], rope_row=case["rope"][case["pos"][s]], eps=case["eps"])
    a.update(over)
    return decode64(a["qkv"], a["qn"], a["kn"], a["rope_row"], a["eps"], kc, vc, int(case["pos"][s]), case["nH"],
                    case["nKV"], case["D"], mut)


def prefill_case(seed, D, R, nKV, plen, n_utt, scales, peaked=False):
    """the inputs of one prefill_attn launch: n_utt utterances of plen rows (raw standard deviation scales[utt])"""
    rng = np.random.default_rng(seed)
    nH = R * nKV
    qn = np.exp(0.3 * rng.standard_normal(D)).astype(np.float32) * np.float32(6.0 if peaked else 1.0)
    kn = np.exp(0.3 * rng.standard_normal(D)).astype(np.float32)
    rope = rope_table(plen + 1, D)
    n = n_utt * plen
    rsc = np.repeat(np.asarray(scales, np.float32), plen)
    rr = np.tile(rope[:plen], (n_utt, 1))[:, None, :]
    rows = np.zeros((n, nH + 2 * nKV, D), np.float32)
    for h in range(nH + nKV):
        rows[:, h] = draw_heads(rng, rsc, qn if h < nH else kn, rr, EPS, D)
    rows[:, nH + nKV:] = rng.standard_normal((n, nKV, D), dtype=np.float32) * rsc[:, None, None]
    return dict(D=D, R=R, nKV=nKV, nH=nH, plen=plen, n_utt=n_utt, qn=qn, kn=kn, rope=rope, eps=EPS,
                qkv=rows.reshape(n_utt, plen, -1))


# ------------------------------------------------------------------------------------------------ the launches
# Every launch of tests/test_gpu_attn_ops.py as the keyword arguments of decode_case / prefill_case (plus the launch
# parameters chunk / kernel), so that the mutation checks of tests/test_attn_ops_ref.py run on the very same inputs.
SCALES = (1e-3, 1.0, 1e3)
LAYOUTS_OTHER = ((128, 1), (128, 4), (64, 1), (64, 2), (64, 4))
N_CTX_SPLIT, N_CTX_OTHER, N_CTX_SEQ = 1088, 576, 1088


def _scales(i, S):
    return tuple(SCALES[(i + s) % 3] for s in range(S))


def split_launches(D, R, chunk, peaked=False):
    """k_attn: three slots with different split counts per launch, nKV = 2"""
    if peaked:
        groups = [(63, 129, 1024)]
    elif (D, R) != (128, 2):
        groups = [(p, 200, 512) for p in (0, 31, 32, 63, 64, 65)]
    elif chunk == 64:     # split counts 1 | 2, 3 | 8, 9, 16, 17
        low, mid, high = (0, 1, 15, 16, 31, 32, 62, 63), (64, 65, 127, 128, 129), (511, 512, 513, 1023, 1024)
        groups = [(low[i], mid[i % 5], high[i % 5]) for i in range(8)]
    else:                 # split counts 1 | 2 | 3, 8, 9
        groups = [(0, 128, 1023), (127, 129, 1024), (0, 255, 256)]
    n_ctx = N_CTX_SPLIT if (D, R) == (128, 2) else N_CTX_OTHER
    return [dict(kernel="k_attn", chunk=chunk, seed=1000 * D + 100 * R + chunk + 7 * i + (5 if peaked else 0), D=D, R=R,
                 nKV=2, n_ctx=n_ctx, poss=g, scales=_scales(i + 1, 3), peaked=peaked) for i, g in enumerate(groups)]


def seq_launches(peaked=False):
    """k_attn_seq: S = 4, nKV = 3"""
    poss = (0, 3, 4, 11, 12, 15, 16, 47, 48, 63, 64, 65, 127, 128, 191, 192, 200, 576, 1024, 2)
    groups = [(15, 200, 576, 1024)] if peaked else [poss[i::5] for i in range(5)]
    return [dict(kernel="k_attn_seq", seed=31000 + 7 * i + (5 if peaked else 0), D=128, R=2, nKV=3, n_ctx=N_CTX_SEQ,
                 poss=g, scales=_scales(i + 1, 4), peaked=peaked) for i, g in enumerate(groups)]


TAB = dict(rows=40, ld=16, col=3, row0=7, tok=(21, 5, 32, 5, 0))     # non-monotonic, slots 1 and 3 share a token


def small_launches(n_ctx, tab=False, peaked=False):
    """k_attn_small: S = 5, nKV = 3, every position of the context"""
    if peaked:
        groups = [(0, 4, 8, 12, 15)]
    elif n_ctx == 16:
        groups = [(0, 4, 8, 12, 15), (1, 5, 9, 13, 3), (2, 6, 10, 14, 7), (3, 7, 11, 15, 0)]
    else:
        groups = [(0, 2, 4, 6, 8), (1, 3, 5, 7, 8)]
    return [dict(kernel="k_attn_small", seed=52000 + 100 * n_ctx + 7 * i + (3 if tab else 0) + (5 if peaked else 0), D=128,
                 R=2, nKV=3, n_ctx=n_ctx, poss=g, scales=_scales(i + 1, 5), peaked=peaked, tab=TAB if tab else None)
            for i, g in enumerate(groups)]


def make(launch):
    """the decode_case of a launch"""
    kw = {k: v for k, v in launch.items() if k not in ("kernel", "chunk")}
    return decode_case(**kw)


def n_exp_of(kernel, pos):
    """the number of __expf factors in a weight (docstring: exp_term)"""
    return {"k_attn": 1, "k_prefill_attn": 1, "k_attn_small": 0, "k_attn_seq": 2 + pos // 64}[kernel]
