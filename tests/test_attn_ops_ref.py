"""CPU checks of tests/attn_ops_ref.py, the reference and tolerance of tests/test_gpu_attn_ops.py (no GPU):
  * the float32 re-evaluations of the reference, in the four summation structures the kernels use, stay inside the
    tolerance; their needs (printed) define C_TOL_ATTN = 4 x the largest;
  * the generator's accepted head vectors round to the same f16 values in float32 and float64; the float32
    prologue's distance from float64 (printed) defines MARGIN = 4 x the largest;
  * mutation checks: each defect a kernel could have is applied to the REFERENCE on the inputs of the GPU launch
    designed for it, and must move some output element by at least 8 x that element's tolerance or change a cache
    row's bits -- the proof that the GPU tests would notice a kernel with that defect.
"""
import numpy as np
import pytest

import attn_ops_ref as A

U = A.U


# ------------------------------------------------------------------------------------------------ generator
def test_generator_rounds_alike():
    rng = np.random.default_rng(2024)
    worst, n_vec = 0.0, 0
    for D in (64, 128):
        rope = A.rope_table(1100, D)
        for scale in A.SCALES:
            w = np.exp(0.3 * rng.standard_normal(D)).astype(np.float32)
            rows = rope[rng.integers(0, 1100, 667)]
            raw = A.draw_heads(rng, np.full(667, scale, np.float32), w, rows[:, None, :], A.EPS, D)
            y64, mag = A.prologue64(raw, w, rows, A.EPS, D)
            y32 = A.prologue32(raw, w, rows, A.EPS, D)
            assert np.array_equal(y32.astype(np.float16).view(np.uint16), y64.astype(np.float16).view(np.uint16)), \
                f"an accepted vector rounds differently in float32 (D {D}, scale {scale})"
            worst = max(worst, float(np.max(np.abs(y32.astype(np.float64) - y64) / (U * mag))))
            n_vec += 667
    print(f"float32 prologue vs float64 over {n_vec} accepted vectors: {worst:.2f} u mag (MARGIN {A.MARGIN})")
    assert 4.0 * worst <= A.MARGIN


def test_generator_is_deterministic_and_rejects():
    rng = np.random.default_rng(5)
    w = np.ones(128, np.float32)
    rope = A.rope_table(4, 128)[[3]]
    # acceptance rate of plain draws: about one in three
    cand = rng.standard_normal((600, 128), dtype=np.float32)
    y, mag = A.prologue64(cand, w, rope, A.EPS, 128)
    rate = float((A.boundary_dist(y) > A.MARGIN * U * mag).all(-1).mean())
    print(f"acceptance rate {rate:.2f}")
    assert 0.1 < rate < 0.6
    a = A.make(A.small_launches(9)[0])
    b = A.make(A.small_launches(9)[0])
    assert all(np.array_equal(a[k], b[k]) for k in ("qkv", "kc", "vc", "qn", "kn", "rope"))


# ------------------------------------------------------------------------------------------------ float32 re-evaluations
STRUCTURES = ("sequential", "tree", "online", "split")


@pytest.fixture(scope="module")
def f32_needs():
    """need of every structure over contexts 1 .. 1,088 positions, both head widths, plain and peaked scores"""
    needs = {s: 0.0 for s in STRUCTURES}
    worst = 0.0
    for D, R in ((128, 2), (64, 4)):
        for peaked in (False, True):
            case = A.decode_case(77 + D + peaked, D, R, 1, 1088, (0, 15, 64, 200, 513, 1087), (1.0, 1e-3, 1e3, 1.0, 1.0, 1.0),
                                 peaked=peaked)
            for s in range(case["S"]):
                ops = []
                ref = A.decode_ref(case, s, mut=dict(operands=ops))
                for h, (q, K, V) in enumerate(ops):
                    for st in STRUCTURES:
                        got = A.eval32(st, q, K, V, D).astype(np.float64)
                        err = np.abs(got - ref["out"][h])
                        needs[st] = max(needs[st], float(np.max(err / (U * ref["allow"][h]))))
                        worst = max(worst, float(np.max(err / (A.C_TOL_ATTN * U * ref["allow"][h]))))
    return needs, worst


def test_f32_reevaluations(f32_needs):
    needs, worst = f32_needs
    print("float32 re-evaluation needs: " + ", ".join(f"{k} {v:.2f}" for k, v in needs.items()) +
          f" => C_TOL_ATTN >= {4 * max(needs.values()):.2f} (is {A.C_TOL_ATTN})")
    assert worst <= 1.0, "a float32 re-evaluation outside the tolerance"
    assert 4.0 * max(needs.values()) <= A.C_TOL_ATTN * 1.0001, "C_TOL_ATTN is below 4 x the measured need"
    assert A.C_TOL_ATTN <= 4.0 * max(needs.values()) * 1.05, "C_TOL_ATTN is not the measured constant"


def test_eval32_structures_agree_with_reference_exactly_on_one_position():
    case = A.decode_case(3, 128, 2, 1, 16, (0,), (1.0,))
    ops = []
    ref = A.decode_ref(case, 0, mut=dict(operands=ops))
    for h, (q, K, V) in enumerate(ops):
        for st in STRUCTURES:
            assert np.array_equal(A.eval32(st, q, K, V, 128).astype(np.float64), ref["out"][h])   # p = 1: out = V


# ------------------------------------------------------------------------------------------------ mutation checks
def pick(launches, want):
    """(case, launch, slot) of the first launch with a slot satisfying want(pos, scale)"""
    for L in launches:
        for s, (pos, sc) in enumerate(zip(L["poss"], L["scales"])):
            if want(pos, sc):
                return A.make(L), L, s
    raise AssertionError("no launch designed for this mutation")


def moved(case, L, s, mut=None, **over):
    """how far the mutated reference lies from the true one: (max |diff| / tol, cache row bits changed)"""
    ref = A.decode_ref(case, s)
    bad = A.decode_ref(case, s, mut=mut, **over)
    t = A.tol(ref, A.n_exp_of(L["kernel"], int(case["pos"][s])))
    d = np.abs(bad["out"] - ref["out"])
    ratio = float(np.max(np.where(np.isfinite(d), d, np.inf) / t))
    bits = not (np.array_equal(A.h16bits(bad["k_new"]), A.h16bits(ref["k_new"])) and
                np.array_equal(A.h16bits(bad["v_new"]), A.h16bits(ref["v_new"])))
    return ratio, bits


def detected(name, ratio, bits):
    print(f"{name}: moves an output element by {ratio:.3g} x its tolerance" + (", changes the cache row" if bits else ""))
    assert ratio >= 8.0 or bits, f"{name}: the tests would not notice (only {ratio:.3g} x the tolerance)"


LONG = dict(split64=lambda: A.split_launches(128, 2, 64), split128=lambda: A.split_launches(128, 2, 128),
            seq=lambda: A.seq_launches())
not_huge = lambda sc: sc <= 1.0      # the 1e3 slots' own new V row dominates their outputs


@pytest.mark.parametrize("fam", ["split64", "split128", "seq", "small16", "small9"])
def test_mut_last_position_dropped(fam):
    launches = LONG[fam]() if fam in LONG else A.small_launches(int(fam[5:]))
    top = max(p for L in launches for p in L["poss"])
    case, L, s = pick(launches, lambda pos, sc: pos == top and not_huge(sc))
    detected(f"{fam} pos {top}: last position dropped", *moved(case, L, s, mut=dict(drop=[top])))


@pytest.mark.parametrize("fam", ["split64", "split128", "seq"])
def test_mut_chunk_edge_dropped(fam):
    """every position 64 k (128 k) <= pos of the longest slot, one at a time"""
    case, L, s = pick(LONG[fam](), lambda pos, sc: pos == 1024 and not_huge(sc))
    for step in (64, 128):
        for j in range(step, 1025, step):
            detected(f"{fam} pos 1024: position {j} dropped", *moved(case, L, s, mut=dict(drop=[j])))
    # and around the first edge of a short context
    case, L, s = pick(LONG[fam](), lambda pos, sc: 128 <= pos <= 200 and not_huge(sc))
    for j in (63, 64, 127, 128):
        detected(f"{fam} pos {case['pos'][s]}: position {j} dropped", *moved(case, L, s, mut=dict(drop=[j])))


@pytest.mark.parametrize("fam", ["split64", "seq", "small16"])
def test_mut_stale_row(fam):
    launches = LONG[fam]() if fam in LONG else A.small_launches(16)
    case, L, s = pick(launches, lambda pos, sc: pos >= 8 and sc == 1.0)
    pos = int(case["pos"][s])
    ratio, _ = moved(case, L, s, mut=dict(stale=True))            # the harness's poison: NaN
    detected(f"{fam} pos {pos}: row pos read from the (poisoned) cache", ratio, False)
    rng = np.random.default_rng(1)                                # and a plausible stale row: caught by the values
    for c in ("kc", "vc"):
        case[c][s, :, pos] = A.h16bits(rng.standard_normal((case["nKV"], case["D"]), dtype=np.float32))
    ratio, _ = moved(case, L, s, mut=dict(stale=True))
    detected(f"{fam} pos {pos}: row pos read from a stale cache row", ratio, False)


@pytest.mark.parametrize("chunk", [64, 128])
def test_mut_split_combine(chunk):
    case, L, s = pick(A.split_launches(128, 2, chunk), lambda pos, sc: pos == 1024 and not_huge(sc))
    nsplit = 1024 // chunk + 1
    for sp in range(nsplit):
        detected(f"chunk {chunk}: split {sp} left out", *moved(case, L, s, mut=dict(split_drop=(chunk, sp))))
    # weight 1 in place of exp(m_s - m): no defect for a head whose maximum lies in that split, so per split the
    # best-placed head decides (no split holds the maximum of all four heads)
    for sp in range(nsplit):
        detected(f"chunk {chunk}: split {sp} combined with weight 1", *moved(case, L, s, mut=dict(split_w1=(chunk, sp))))
    # the peaked launch: split maxima tens apart
    case, L, s = pick(A.split_launches(128, 2, chunk, peaked=True), lambda pos, sc: pos == 129)
    for sp in range(129 // chunk + 1):
        ratio, bits = moved(case, L, s, mut=dict(split_w1=(chunk, sp)))
        print(f"peaked chunk {chunk}: split {sp} combined with weight 1: {ratio:.3g} x")
        best = ratio if sp == 0 else max(best, ratio)
    assert best >= 8.0


@pytest.mark.parametrize("fam", ["128x2", "128x4", "64x2", "64x4", "seq", "small", "small_tab"])
def test_mut_kv_head_mapping(fam):
    if fam == "seq":
        launches = A.seq_launches()
    elif fam.startswith("small"):
        launches = A.small_launches(16, tab=fam.endswith("tab"))
    else:
        launches = A.split_launches(*(int(v) for v in fam.split("x")), 64)
    for L in launches[:2]:
        case = A.make(L)
        for s in range(case["S"]):
            detected(f"{fam} pos {case['pos'][s]}: q head h -> kv head h % nKV", *moved(case, L, s, mut=dict(kvmap="mod")))


def all_layout_launches():
    out = [A.split_launches(128, 2, 64)[3], A.seq_launches()[2], A.small_launches(16)[1]]
    return out + [A.split_launches(D, R, 128)[4] for D, R in A.LAYOUTS_OTHER]


def test_mut_prologue():
    """RoPE row pos +- 1, interleaved pairing, 1 / sqrt(D) left out: every layout, every slot"""
    for L in all_layout_launches():
        case = A.make(L)
        tag = f"{L['kernel']} ({L['D']}, {L['R']})"
        for s in range(case["S"]):
            pos = int(case["pos"][s])
            for dp in (-1, 1):
                if pos + dp >= 0:
                    ratio, bits = moved(case, L, s, rope_row=case["rope"][pos + dp])
                    detected(f"{tag} pos {pos}: RoPE row pos {dp:+d}", ratio, bits)
                    assert bits and (pos == 0 or ratio >= 8.0)
            if pos > 0:   # (row 0 of the table is the identity rotation: the pairing does not matter there)
                ratio, bits = moved(case, L, s, mut=dict(interleaved=True))
                detected(f"{tag} pos {pos}: interleaved RoPE pairing", ratio, bits)
                assert bits and ratio >= 8.0
                detected(f"{tag} pos {pos}: 1 / sqrt(D) left out", *moved(case, L, s, mut=dict(no_scale=True)))


def test_mut_eps():
    """eps left out, on the slots whose raw rows have magnitude 1e-3 (mean(x^2) ~ eps)"""
    for L in all_layout_launches():
        case = A.make(L)
        hit = 0
        for s in range(case["S"]):
            if L["scales"][s] == 1e-3:
                ratio, bits = moved(case, L, s, eps=0.0)
                detected(f"{L['kernel']} ({L['D']}, {L['R']}) pos {case['pos'][s]}: eps left out", ratio, bits)
                assert bits
                hit += 1
        assert hit


def test_mut_qkv_tab():
    """the table row taken from tab_col +- 1, or without tab_row0"""
    for L in A.small_launches(16, tab=True) + A.small_launches(9, tab=True):
        case = A.make(L)
        S, ld, col, row0 = case["S"], case["tab_ld"], case["tab_col"], case["tab_row0"]
        good = A.tab_rows(case["tab_tok"], S, ld, col, row0)
        assert np.array_equal(case["table"][good], case["qkv"])
        for name, rows in (("tab_col - 1", A.tab_rows(case["tab_tok"], S, ld, col - 1, row0)),
                           ("tab_col + 1", A.tab_rows(case["tab_tok"], S, ld, col + 1, row0)),
                           ("no tab_row0", A.tab_rows(case["tab_tok"], S, ld, col, 0))):
            assert rows.max() < case["table"].shape[0]
            for s in range(S):
                ratio, bits = moved(case, L, s, qkv=case["table"][rows[s]])
                detected(f"qkv_tab pos {case['pos'][s]}: {name}", ratio, bits)
                assert bits


def test_mut_prefill():
    """the prefill's rows are decode64 at their own position: the defects above on its last row, plus a row that
    attends to a later one"""
    for D, R in ((128, 2),) + A.LAYOUTS_OTHER:
        pc = A.prefill_case(900 + D + R, D, R, 2, 16, 3, A.SCALES)
        for u in range(3):
            ref = A.prefill64(pc["qkv"][u], pc["qn"], pc["kn"], pc["rope"], pc["eps"], pc["nH"], 2, D)
            t = A.tol(ref, 1)
            muts = [("last position dropped", dict(drop=[15]), {}), ("interleaved", dict(interleaved=True), {}),
                    ("1 / sqrt(D) left out", dict(no_scale=True), {}), ("RoPE row + 1", None, dict(rope=pc["rope"][1:]))]
            if R > 1:
                muts.append(("kv head h % nKV", dict(kvmap="mod"), {}))
            if A.SCALES[u] == 1e-3:
                muts.append(("eps left out", None, dict(eps=0.0)))
            for name, mut, over in muts:
                a = dict(rope=pc["rope"], eps=pc["eps"])
                a.update(over)
                bad = A.prefill64(pc["qkv"][u], pc["qn"], pc["kn"], a["rope"], a["eps"], pc["nH"], 2, D, mut)
                ratio = float(np.max(np.abs(bad["out"][15] - ref["out"][15]) / t[15]))
                bits = not np.array_equal(A.h16bits(bad["k_new"]), A.h16bits(ref["k_new"]))
                detected(f"prefill ({D}, {R}) utterance {u}: {name}", ratio, bits)
            # row i over rows 0..i+1 (a causal mask off by one): row 14 computed as row 15's keys would have it
            kc = np.transpose(ref["k_new"], (1, 0, 2))
            vc = np.transpose(ref["v_new"], (1, 0, 2))
            good = A.decode64(pc["qkv"][u][14], pc["qn"], pc["kn"], pc["rope"][14], pc["eps"], kc, vc, 14, pc["nH"], 2, D)
            leak = A.decode64(pc["qkv"][u][14], pc["qn"], pc["kn"], pc["rope"][14], pc["eps"], kc, vc, 15, pc["nH"], 2, D,
                              dict(stale=True))
            assert np.array_equal(good["out"], ref["out"][14])
            ratio = float(np.max(np.abs(leak["out"] - good["out"]) / t[14]))
            detected(f"prefill ({D}, {R}) utterance {u}: row 14 sees row 15", ratio, False)
