"""The 1.7B layout (a 2,048 / 6,144 talker over a 1,024 / 3,072 code predictor behind code_pred.mtp_proj) on the batched
matrix-core stack: from 4 slots its projections are MFMA GEMMs (K = 2,048 with the SwiGLU epilogue, K = 6,144 as
split-K slabs), its norms the wide k_resid_norm, its code-predictor passes start from rows of the projected table
(passes 1..15, handed over by the selection launch) or one mtp_proj GEMM (pass 0).

Model: wide17 (tools/q3t_synth.c), the real 1.7B widths and head layouts at 2 + 2 layers.  Reference: the CPU oracle
(no fixture of the reference project covers the 1.7B path).  Tolerances are those the existing 1.7B tests state for
the same quantities: 2e-3 relative on the talker step (test_full17_shapes_generate_and_vocoder), 5e-2 absolute on
teacher-forced code-predictor logits and on greedy near-ties (test_codepred_frame_matches_oracle), check_decisions'
defaults with max_off_frac = 0.05 on generated codes.
"""
import os
import sys

import numpy as np
import pytest

from mm17_inputs import CP_MAX_TIE_FRAC, CP_SLOTS, CP_TIE_TOL, cp_frame_inputs
from oracle_py import Oracle
from q3t_testutil import REPO, check_decisions, check_token, prompt, rel_err, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu


def _engine(cfg, env=None, **kw):
    import q3t
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return q3t.Engine(synth_dir(cfg)[0], None, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def wide17():
    tts, tok = synth_dir("wide17")
    eng = _engine("wide17", max_slots=64, max_ctx=64)
    orc = Oracle(tts, tok)
    yield eng, orc
    eng.close()
    orc.close()


def test_decode_family_reports_the_matrix_core_stack(wide17):
    eng, _ = wide17
    assert eng.cfg["has_mtp"] == 1 and (eng.cfg["hidden"], eng.cfg["intermediate"]) == (2048, 6144)
    assert eng.decode_family(1) == 0
    assert eng.decode_family(4) == 1 and eng.decode_family(64) == 1
    import q3t
    for n in (0, 65):
        with pytest.raises(q3t.Q3TError):
            eng.decode_family(n)
    off = _engine("wide17", env={"Q3T_MM17": "0"}, max_slots=4, max_ctx=64)
    try:
        assert off.decode_family(4) == 0
    finally:
        off.close()
    tiny = _engine("tiny", max_slots=4, max_ctx=64)
    try:
        assert tiny.decode_family(4) in (1, 2)
    finally:
        tiny.close()


# ---------------------------------------------------------------------------------------------- talker step
N_STEPS = 3


@pytest.fixture(scope="module")
def talker_ref(wide17):
    """64 slots, each with a start position of its own in 0..9, inputs of its own for its history and its N_STEPS
    checked steps, and an oracle KV of its own: the oracle's hidden state and logits of the checked steps.  Computed
    once; a case of n slots uses the first n."""
    _, orc = wide17
    H = orc.cfg["hidden"]
    rng = np.random.default_rng(17)
    start = rng.integers(0, 10, 64)
    start[:4] = [0, 9, 3, 6]   # the 4-slot case sees both ends
    x = (rng.standard_normal((64, 12, H)) * 0.5).astype(np.float32)   # x[s][p]: slot s's input at position p
    hid = np.zeros((64, N_STEPS, H), np.float32)
    lg = np.zeros((64, N_STEPS, orc.cfg["codec_vocab"]), np.float32)
    for s in range(64):
        kv = orc.kv_new(64, 0)
        for p in range(start[s] + N_STEPS):
            h, l = orc.talker_step(kv, x[s, p], p)
            if p >= start[s]:
                hid[s, p - start[s]], lg[s, p - start[s]] = h, l
        orc.kv_free(kv)
    return start, x, hid, lg


@pytest.mark.parametrize("slots", [4, 33, 64])
def test_talker_step_matches_oracle(wide17, talker_ref, slots):
    eng, _ = wide17
    start, x, hid, lg = talker_ref
    start = start[:slots]
    idx = np.arange(slots)
    # each slot's history (positions below its start) through the same batched step: a slot that has reached its start
    # repeats its last history position (the same K/V rows again)
    for t in range(int(start.max())):
        pos = np.minimum(t, np.maximum(start - 1, 0))
        eng.talker_forward(x[idx, pos], pos)
    worst_h = worst_l = 0.0
    for j in range(N_STEPS):
        pos = start + j
        hg, lgg = eng.talker_forward(x[idx, pos], pos)
        for s in range(slots):
            eh, el = rel_err(hg[s], hid[s, j]), rel_err(lgg[s], lg[s, j])
            worst_h, worst_l = max(worst_h, eh), max(worst_l, el)
    print(f"wide17 talker step, {slots} slots: worst rel err hidden {worst_h:.3g} logits {worst_l:.3g}")
    assert worst_h < 2e-3 and worst_l < 2e-3, (slots, worst_h, worst_l)


# ---------------------------------------------------------------------------------------------- code-predictor frame
@pytest.mark.parametrize("temperature", [0.0, 0.9])
@pytest.mark.parametrize("slots", CP_SLOTS)
def test_codepred_frame_matches_oracle(wide17, slots, temperature):
    """pass 0 through the mtp_proj GEMM, passes 1..15 from the projected table: logits teacher-forced on the GPU's own
    codes, every greedy code the oracle's argmax or a near-tie, near-ties rare"""
    eng, orc = wide17
    hid, cb0 = cp_frame_inputs(eng.cfg["hidden"])
    hid, cb0 = hid[:slots], cb0[:slots]
    codes, lg = eng.codepred_frame(hid, cb0, temperature=temperature, top_k=50, seed=4, frame=2, want_logits=True)
    off = 0
    worst = 0.0
    for s in range(slots):
        ol = orc.cp_frame_forced(hid[s], int(cb0[s]), codes[s])
        worst = max(worst, float(np.abs(lg[s] - ol).max()))
        if temperature <= 0:
            off += sum(check_token(ol[i], int(codes[s, i]), 0.0, 0, 0.0, tol_logit=CP_TIE_TOL) for i in range(15))
    print(f"wide17 code-predictor frame, {slots} slots T={temperature}: worst logit err {worst:.3g}, {off} near-ties")
    assert worst < 5e-2, worst
    assert off <= CP_MAX_TIE_FRAC * slots * 15, (off, slots * 15)


# ---------------------------------------------------------------------------------------------- prefill
def test_prefill_rows_equal_the_4_slot_step_bit_exact(wide17):
    """the header's contract at K = 2,048 / 6,144: a prefill row run as a 4-slot step's family equals that step"""
    eng, _ = wide17
    H = eng.cfg["hidden"]
    x = (np.random.default_rng(23).standard_normal((2, 6, H)) * 0.5).astype(np.float32)
    hp, lp = eng.talker_prefill(x, family_slots=4)
    x4 = np.concatenate([x, x[:, ::-1]])   # slots 2 and 3: other rows alongside
    hr = np.zeros_like(x)
    for t in range(6):
        h, lr = eng.talker_forward(x4[:, t], [t] * 4)
        hr[:, t] = h[:2]
    assert np.array_equal(hp, hr), float(np.abs(hp - hr).max())
    assert np.array_equal(lp, lr[:2]), float(np.abs(lp - lr[:2]).max())


# ---------------------------------------------------------------------------------------------- generate / queue
def _prompts(n):
    base = prompt("wide17")
    return [base[:4] + [(t + 37 * i) % 900 + 20 for t in base[4:]] for i in range(n)]


@pytest.mark.parametrize("slots", [4, 8])
def test_generate_matches_oracle(wide17, slots):
    eng, orc = wide17
    H = eng.cfg["hidden"]
    prompts = _prompts(slots)
    spk = [np.zeros(H, np.float32)] * slots
    outs = eng.generate(prompts, speakers=spk, max_len=16, temperature=0.9, top_k=50, seed=31, force_frames=16)
    for i, out in enumerate(outs):
        assert out.shape == (16, 16)
        n_off, n_dec, worst = check_decisions(orc, prompts[i], spk[i], out, max_len=16, force_frames=16,
                                              temperature=0.9, top_k=50, seed=31, utt=i, max_off_frac=0.05)
        print(f"wide17 slots={slots} utt {i}: {n_dec - n_off}/{n_dec} exact, worst {worst:.3g}")


def test_queue_is_admission_invariant_and_starts_as_generate():
    eng = _engine("wide17", max_slots=4, max_ctx=64)
    try:
        assert eng.decode_family(4) == 1
        H = eng.cfg["hidden"]
        n_utt = 8
        prompts = _prompts(n_utt)
        rng = np.random.default_rng(2)
        spk = [(rng.standard_normal(H) * 0.02).astype(np.float32) for _ in range(n_utt)]
        kw = dict(max_len=16, temperature=0.9, top_k=50, seed=31)
        a = eng.generate_queue(prompts, speakers=spk, max_active=4, **kw)
        b = eng.generate_queue(prompts, speakers=spk, max_active=1, **kw)
        assert all(0 < len(c) <= 16 for c in a)
        for u in range(n_utt):
            assert np.array_equal(a[u], b[u]), (u, len(a[u]), len(b[u]))
        g = eng.generate(prompts[:4], speakers=spk[:4], **kw)
        for u in range(4):
            assert np.array_equal(a[u], g[u]), (u, len(a[u]), len(g[u]))
    finally:
        eng.close()
