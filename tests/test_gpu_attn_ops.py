"""The decode and prefill attention kernels behind attn_decode() and prefill_attn() (csrc/attn.hip: k_attn, k_attn_seq,
k_attn_small, k_prefill_attn), one launch at a time through the test-only shim tests/attn_ops/libq3t_attn_ops.so,
against the float64 reference and tolerance of tests/attn_ops_ref.py (whose launch tables this file runs, and on whose
inputs tests/test_attn_ops_ref.py proves that a defective kernel would be noticed).

Every launch: each slot at its own position; cache rows < pos random f16, rows >= pos -- row pos included -- f16 NaN
poison (the kernels clamp their loads to row pos and mask them: leaked poison makes the output NaN); outputs, `part`,
`ticket` and the caches between guard regions, outputs and `part` prefilled with NaN sentinels.  Checked after the
launch: every output element written and within tolerance, cache row pos equal to the reference bit for bit, every
other cache byte unchanged, guards intact, ticket[] all zero; then a second launch on the same buffers (row pos now
real, `part` dirty) must give the same output bits.  Before every launch the test asserts on the host that its own
buffers satisfy the launcher's contract.

Every test prints its need (attn_ops_ref.need: what the f16 outputs show of the kernel's f32 error, in the units of
C_TOL_ATTN, after and before the derived exp_term is taken off); test_zz_measured prints the largest per kernel.
"""
import ctypes as C

import numpy as np
import pytest

import attn_ops_ref as A
from attn_ops_lib import AttnDesc, PrefillAttnDesc, load
from voc_ops_ref import worst_ratio

pytestmark = pytest.mark.gpu

G = 4096                                    # guard elements before and after every buffer
SENT32, SENT16 = 0x7FC00123, A.POISON
NEED = {}


@pytest.fixture(scope="module")
def ops():
    return load()


class GuardBuf:
    """a device array with G guard elements of a sentinel on both sides"""

    def __init__(self, ops, body, sent):
        body = np.ascontiguousarray(body)
        self.dt, self.n, self.sent = body.dtype, body.size, sent
        host = np.full(self.n + 2 * G, sent, self.dt)
        host[G:G + self.n] = body.reshape(-1)
        self.dev = ops.DevBuf(host)
        self.p = self.dev.p + G * host.itemsize

    def fetch(self, what):
        a = self.dev.get(self.dt, self.n + 2 * G)
        assert (a[:G] == self.sent).all() and (a[G + self.n:] == self.sent).all(), f"{what}: written outside the buffer"
        return a[G:G + self.n]


def report(kernel, name, ratio, need):
    NEED[kernel] = np.maximum(NEED.get(kernel, np.zeros(2)), need)
    print(f"{name}: worst |err| / tol = {ratio:.3f}, need = {need[0]:.2f} (before exp_term {need[1]:.2f}; "
          f"C_TOL_ATTN {A.C_TOL_ATTN})")


def f16vals(bits):
    return bits.view(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------------ decode
def run_decode(ops, L):
    """one attn_decode launch of the table (twice); returns (worst |err| / tol, need)"""
    case = A.make(L)
    kernel, chunk = L["kernel"], L.get("chunk", 64)
    S, nH, nKV, D, n_ctx, pos = case["S"], case["nH"], case["nKV"], case["D"], case["n_ctx"], case["pos"]
    R, QKV = nH // nKV, (nH + 2 * nKV) * D
    split = kernel == "k_attn"
    max_splits = (n_ctx + chunk - 1) // chunk if split else 1
    n_part = S * nH * max_splits * (D + 2)
    tab = "table" in case
    # ---- the launcher's contract, on the host
    assert S <= 5 and nKV <= 3 and n_ctx <= 1088
    assert (pos >= 0).all() and (pos < n_ctx).all()
    assert case["rope"].shape == (case["rope"].shape[0], D) and case["rope"].shape[0] > pos.max()
    assert D in (64, 128) and R in (1, 2, 4) and nH == R * nKV
    assert case["kc"].shape == case["vc"].shape == (S, nKV, n_ctx, D)
    if split:
        assert chunk in (64, 128) and max_splits * chunk >= n_ctx and max_splits <= 160
    else:
        assert (D, R) == (128, 2) and (kernel != "k_attn_small" or n_ctx <= 16)
    if tab:
        idx = np.arange(S) * case["tab_ld"] + case["tab_col"]
        assert idx.max() < case["tab_tok"].size
        rows = case["tab_row0"] + case["tab_tok"].reshape(-1)[idx]
        assert rows.min() >= 0 and rows.max() < case["table"].shape[0] and case["table"].shape[1] == QKV
        assert np.array_equal(case["table"][rows], case["qkv"])
        assert len(set(rows)) < S and (np.diff(rows) < 0).any()       # a shared token, non-monotonic
    # ---- buffers
    qkv = ops.DevBuf(np.full((S, QKV), np.nan, np.float32) if tab else case["qkv"])
    table = ops.DevBuf(case["table"]) if tab else None
    tab_tok = ops.DevBuf(case["tab_tok"]) if tab else None
    qn, kn, rope, posd = (ops.DevBuf(case[k]) for k in ("qn", "kn", "rope", "pos"))
    kc, vc = GuardBuf(ops, case["kc"], SENT16), GuardBuf(ops, case["vc"], SENT16)
    part = GuardBuf(ops, np.full(n_part, SENT32, np.uint32), 0x7FC00456) if split else None
    ticket = GuardBuf(ops, np.zeros(S * nKV, np.uint32), 0xDEADBEEF)
    assert part is None or part.n == S * nH * max_splits * (D + 2)
    assert ticket.n == S * nKV
    d = AttnDesc()
    d.qkv, d.qn, d.kn, d.rope, d.pos, d.kc, d.vc = qkv.p, qn.p, kn.p, rope.p, posd.p, kc.p, vc.p
    d.part, d.ticket = (part.p if split else 0), ticket.p
    d.eps, d.n_ctx, d.S, d.nH, d.nKV, d.D = case["eps"], n_ctx, S, nH, nKV, D
    d.chunk, d.seqk, d.small, d.max_splits = chunk, int(kernel == "k_attn_seq"), int(kernel == "k_attn_small"), max_splits
    if tab:
        d.qkv_tab, d.tab_tok, d.tab_ld, d.tab_col, d.tab_row0 = table.p, tab_tok.p, case["tab_ld"], case["tab_col"], case["tab_row0"]
    # ---- reference
    refs = [A.decode_ref(case, s) for s in range(S)]
    want_k, want_v = case["kc"].copy(), case["vc"].copy()
    for s in range(S):
        want_k[s, :, pos[s]] = A.h16bits(refs[s]["k_new"])
        want_v[s, :, pos[s]] = A.h16bits(refs[s]["v_new"])
    worst, need = 0.0, np.zeros(2)
    first = None
    for run in (1, 2):
        out = GuardBuf(ops, np.full(S * nH * D, SENT16, np.uint16), 0x7E02)
        d.out = out.p
        ops.call("attn_decode", C.byref(d))
        bits = out.fetch(f"run {run}: out").reshape(S, nH, D)
        assert (bits != SENT16).all(), f"run {run}: output elements not written: first at {np.argwhere(bits == SENT16)[0]}"
        got_k = kc.fetch(f"run {run}: K cache").reshape(want_k.shape)
        got_v = vc.fetch(f"run {run}: V cache").reshape(want_v.shape)
        for s in range(S):
            for nm, got, want in (("K", got_k, want_k), ("V", got_v, want_v)):
                assert np.array_equal(got[s, :, pos[s]], want[s, :, pos[s]]), \
                    f"run {run}: {nm} cache row pos {pos[s]} of slot {s} differs from the reference's bits"
        assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v), f"run {run}: a cache byte outside row pos changed"
        assert not ticket.fetch(f"run {run}: ticket").any(), f"run {run}: ticket[] not zero after the launch"
        if split:
            part.fetch(f"run {run}: part")
        if run == 1:
            first = bits
            for s in range(S):
                n_exp = A.n_exp_of(kernel, int(pos[s]))
                got = f16vals(bits[s])
                worst = max(worst, worst_ratio(got, refs[s]["out"], A.tol(refs[s], n_exp)))
                if np.isfinite(got).all():
                    need = np.maximum(need, A.need(got, refs[s], n_exp))
        else:
            assert np.array_equal(bits, first), "the second launch on the same buffers gave other output bits"
    return worst, need


def run_launches(ops, launches, name):
    worst, need = 0.0, np.zeros(2)
    for L in launches:
        w, n = run_decode(ops, L)
        print(f"  {name} pos {tuple(L['poss'])}: worst |err| / tol = {w:.3f}, need = {n[0]:.2f} ({n[1]:.2f})")
        worst, need = max(worst, w), np.maximum(need, n)
    report(launches[0]["kernel"], name, worst, need)
    assert worst <= 1


@pytest.mark.parametrize("chunk", [64, 128])
def test_k_attn_128x2(ops, chunk):
    launches = A.split_launches(128, 2, chunk)
    want = {64: {0, 1, 15, 16, 31, 32, 62, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024},
            128: {0, 127, 128, 129, 255, 256, 1023, 1024}}[chunk]
    assert {p for L in launches for p in L["poss"]} == want
    for L in launches:
        assert len({p // chunk for p in L["poss"]}) == 3, "three slots with different split counts"
    if chunk == 64:
        assert {p // 64 + 1 for p in want} == {1, 2, 3, 8, 9, 16, 17}
    run_launches(ops, launches, f"k_attn (128, 2) chunk {chunk}")


@pytest.mark.parametrize("chunk", [64, 128])
@pytest.mark.parametrize("D,R", A.LAYOUTS_OTHER)
def test_k_attn_layouts(ops, D, R, chunk):
    launches = A.split_launches(D, R, chunk)
    assert {p for L in launches for p in L["poss"]} == {0, 31, 32, 63, 64, 65, 200, 512}
    run_launches(ops, launches, f"k_attn ({D}, {R}) chunk {chunk}")


def test_k_attn_seq(ops):
    launches = A.seq_launches()
    assert {p for L in launches for p in L["poss"]} >= {0, 3, 4, 11, 12, 15, 16, 47, 48, 63, 64, 65, 127, 128, 191, 192,
                                                         200, 576, 1024}
    assert all(len(L["poss"]) == 4 and L["nKV"] == 3 for L in launches)
    run_launches(ops, launches, "k_attn_seq")


@pytest.mark.parametrize("tab", [False, True], ids=["qkv", "qkv_tab"])
@pytest.mark.parametrize("n_ctx", [16, 9])
def test_k_attn_small(ops, n_ctx, tab):
    launches = A.small_launches(n_ctx, tab)
    assert {p for L in launches for p in L["poss"]} == set(range(n_ctx))
    assert all(len(L["poss"]) == 5 and L["nKV"] == 3 for L in launches)
    if tab:
        assert (A.TAB["row0"], A.TAB["ld"], A.TAB["col"], A.TAB["rows"]) == (7, 16, 3, 40)
    run_launches(ops, launches, f"k_attn_small n_ctx {n_ctx}" + (" through qkv_tab" if tab else ""))


@pytest.mark.parametrize("kernel", ["k_attn 64", "k_attn 128", "k_attn_seq", "k_attn_small"])
def test_decode_peaked(ops, kernel):
    """qn x 6: most weights underflow, split / wave maxima tens apart"""
    launches = {"k_attn 64": lambda: A.split_launches(128, 2, 64, peaked=True),
                "k_attn 128": lambda: A.split_launches(128, 2, 128, peaked=True),
                "k_attn_seq": lambda: A.seq_launches(peaked=True),
                "k_attn_small": lambda: A.small_launches(16, peaked=True)}[kernel]()
    run_launches(ops, launches, f"{kernel} peaked")


# ------------------------------------------------------------------------------------------------ prefill
N_CTX_PF, SLOTS_PF, N_SLOT_PF = 24, (4, 0, 2), 5


def run_prefill(ops, D, R, plen, peaked=False):
    nKV, n_utt = 2, 3
    pc = A.prefill_case(7000 + 100 * D + 10 * R + plen + (5 if peaked else 0), D, R, nKV, plen, n_utt, A.SCALES, peaked)
    nH, QKV = pc["nH"], (pc["nH"] + 2 * nKV) * D
    slot = np.asarray(SLOTS_PF, np.int32)
    rng = np.random.default_rng(plen)
    kc0 = np.full((N_SLOT_PF, nKV, N_CTX_PF, D), A.POISON, np.uint16)
    vc0 = np.full((N_SLOT_PF, nKV, N_CTX_PF, D), A.POISON, np.uint16)
    for s in (1, 3):      # other utterances' rows
        kc0[s] = A.h16bits(rng.standard_normal(kc0[s].shape, dtype=np.float32))
        vc0[s] = A.h16bits(rng.standard_normal(vc0[s].shape, dtype=np.float32))
    # ---- the launcher's contract
    assert 1 <= plen <= 16 and plen <= N_CTX_PF and pc["rope"].shape[0] >= plen and pc["rope"].shape[1] == D
    assert len(set(SLOTS_PF)) == n_utt and max(SLOTS_PF) < N_SLOT_PF and D in (64, 128) and R in (1, 2, 4)
    assert pc["qkv"].shape == (n_utt, plen, QKV)
    qkv, qn, kn, rope, slotd = (ops.DevBuf(a) for a in (pc["qkv"], pc["qn"], pc["kn"], pc["rope"], slot))
    kc, vc = GuardBuf(ops, kc0, SENT16), GuardBuf(ops, vc0, SENT16)
    d = PrefillAttnDesc()
    d.qkv, d.qn, d.kn, d.rope, d.kc, d.vc, d.slot = qkv.p, qn.p, kn.p, rope.p, kc.p, vc.p, slotd.p
    d.eps, d.n_ctx, d.n_utt, d.plen, d.nH, d.nKV, d.D = pc["eps"], N_CTX_PF, n_utt, plen, nH, nKV, D
    refs = [A.prefill64(pc["qkv"][u], pc["qn"], pc["kn"], pc["rope"], pc["eps"], nH, nKV, D) for u in range(n_utt)]
    want_k, want_v = kc0.copy(), vc0.copy()
    for u in range(n_utt):
        want_k[slot[u], :, :plen] = A.h16bits(np.transpose(refs[u]["k_new"], (1, 0, 2)))
        want_v[slot[u], :, :plen] = A.h16bits(np.transpose(refs[u]["v_new"], (1, 0, 2)))
    worst, need = 0.0, np.zeros(2)
    first = None
    for run in (1, 2):
        out = GuardBuf(ops, np.full(n_utt * plen * nH * D, SENT16, np.uint16), 0x7E02)
        d.out = out.p
        ops.call("prefill_attn", C.byref(d))
        bits = out.fetch(f"run {run}: out").reshape(n_utt, plen, nH, D)
        assert (bits != SENT16).all(), f"run {run}: output elements not written: first at {np.argwhere(bits == SENT16)[0]}"
        got_k = kc.fetch(f"run {run}: K cache").reshape(want_k.shape)
        got_v = vc.fetch(f"run {run}: V cache").reshape(want_v.shape)
        for u in range(n_utt):
            assert np.array_equal(got_k[slot[u], :, :plen], want_k[slot[u], :, :plen]), f"run {run}: K rows of utterance {u}"
            assert np.array_equal(got_v[slot[u], :, :plen], want_v[slot[u], :, :plen]), f"run {run}: V rows of utterance {u}"
        assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v), \
            f"run {run}: a cache byte outside rows [0, plen) of the utterances' slots changed"
        if run == 1:
            first = bits
            for u in range(n_utt):
                got = f16vals(bits[u])
                assert got.shape == refs[u]["out"].shape == (plen, nH, D)       # every row of every head
                worst = max(worst, worst_ratio(got, refs[u]["out"], A.tol(refs[u], 1)))
                if np.isfinite(got).all():
                    need = np.maximum(need, A.need(got, refs[u], 1))
        else:
            assert np.array_equal(bits, first), "the second launch on the same buffers gave other output bits"
    return worst, need


@pytest.mark.parametrize("D,R", ((128, 2),) + A.LAYOUTS_OTHER)
def test_k_prefill_attn(ops, D, R):
    worst, need = 0.0, np.zeros(2)
    for plen in ((1, 2, 7, 15, 16) if (D, R) == (128, 2) else (1, 16)):
        w, n = run_prefill(ops, D, R, plen)
        print(f"  k_prefill_attn ({D}, {R}) plen {plen}: worst |err| / tol = {w:.3f}, need = {n[0]:.2f} ({n[1]:.2f})")
        worst, need = max(worst, w), np.maximum(need, n)
    report("k_prefill_attn", f"k_prefill_attn ({D}, {R})", worst, need)
    assert worst <= 1


def test_k_prefill_attn_peaked(ops):
    w, n = run_prefill(ops, 128, 2, 16, peaked=True)
    report("k_prefill_attn", "k_prefill_attn (128, 2) plen 16 peaked", w, n)
    assert w <= 1


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    """parameters the launchers must refuse: false with the message, nothing launched (outputs and caches untouched).
    Every buffer is nevertheless as large as the refused parameters would need."""
    S, nKV, D, n_ctx = 2, 2, 128, 128
    f32 = lambda n: ops.DevBuf(np.ones(n, np.float32))
    kc0 = np.full(S * nKV * n_ctx * D, A.POISON, np.uint16)
    kc, vc = GuardBuf(ops, kc0, SENT16), GuardBuf(ops, kc0, SENT16)
    out = GuardBuf(ops, np.full(S * 16 * 8 * D, SENT16, np.uint16), 0x7E02)
    qkv, qn, kn, rope = f32(S * 16 * 12 * D), f32(D), f32(D), f32(n_ctx * D)
    posd = ops.DevBuf(np.zeros(S, np.int32))
    slotd = ops.DevBuf(np.arange(S, dtype=np.int32))
    part = GuardBuf(ops, np.full(S * 8 * 161 * (D + 2), SENT32, np.uint32), 0x7FC00456)
    ticket = GuardBuf(ops, np.zeros(S * nKV, np.uint32), 0xDEADBEEF)

    def dec(**kw):
        d = AttnDesc()
        d.qkv, d.qn, d.kn, d.rope, d.pos, d.kc, d.vc, d.out = qkv.p, qn.p, kn.p, rope.p, posd.p, kc.p, vc.p, out.p
        d.part, d.ticket, d.eps = part.p, ticket.p, A.EPS
        d.n_ctx, d.S, d.nH, d.nKV, d.D, d.chunk, d.max_splits = n_ctx, S, 2 * nKV, nKV, D, 64, 2
        for k, v in kw.items():
            setattr(d, k, v)
        return "attn_decode", d

    def pre(**kw):
        d = PrefillAttnDesc()
        d.qkv, d.qn, d.kn, d.rope, d.kc, d.vc, d.slot, d.out = qkv.p, qn.p, kn.p, rope.p, kc.p, vc.p, slotd.p, out.p
        d.eps, d.n_ctx, d.n_utt, d.plen, d.nH, d.nKV, d.D = A.EPS, n_ctx, S, 16, 2 * nKV, nKV, D
        for k, v in kw.items():
            setattr(d, k, v)
        return "prefill_attn", d

    cases = [("small with n_ctx 17", dec(small=1, n_ctx=17), "n_ctx <= 16"),
             ("R = 3", dec(nH=3 * nKV), "q/kv head ratio must be 1, 2 or 4"),
             ("chunk 32", dec(chunk=32, max_splits=4), "split buffers too small"),
             ("max_splits * chunk < n_ctx", dec(max_splits=1), "split buffers too small"),
             ("max_splits 161", dec(max_splits=161), "split buffers too small"),
             ("null part", dec(part=0), "split buffers too small"),
             ("prefill plen 0", pre(plen=0), "prefill_attn: bad parameters"),
             ("prefill plen 17", pre(plen=17), "prefill_attn: bad parameters"),
             ("prefill null slot", pre(slot=0), "prefill_attn: bad parameters"),
             ("prefill R = 3", pre(nH=3 * nKV), "prefill_attn: unsupported head layout")]
    for name, (fn, d), text in cases:
        rc, msg = ops.call_rc(fn, C.byref(d))
        assert rc != 0 and text in msg, f"{name}: rc {rc}, message {msg!r}"
        assert (out.fetch(name) == SENT16).all(), f"{name}: the output was written"
        assert np.array_equal(kc.fetch(name), kc0) and np.array_equal(vc.fetch(name), kc0), f"{name}: the cache was written"
        assert (part.fetch(name) == SENT32).all() and not ticket.fetch(name).any(), f"{name}: part / ticket written"
    # the same parameters without the defect are accepted (the refusals above are the defect's, not the harness's)
    fn, d = dec()
    ops.call(fn, C.byref(d))
    assert (out.fetch("accepted")[:S * 2 * nKV * D] != SENT16).all()


def test_zz_measured():
    """(prints) the largest need each kernel showed in this run"""
    print("need per kernel (before exp_term): " + ", ".join(f"{k} {v[0]:.2f} ({v[1]:.2f})" for k, v in sorted(NEED.items())) +
          f" (C_TOL_ATTN {A.C_TOL_ATTN}, defined on the CPU)")
