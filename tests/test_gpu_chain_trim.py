"""The one-slot role kernels (k_tk_roles, k_cp_roles) after the trim of their role bodies -- no timeline stamps in the
release library, DPP reduction steps folded into their adds (the two files are compiled without the SLP vectoriser, which
also used to keep rms_to_f16's products from fusing with their f16 conversions: a build that lets them fuse fails here),
non-temporal talker weight loads -- against the two paths that the trim leaves untouched: the all-role persistent kernels (Q3T_TK_ROLES=0 Q3T_CP_ROLES=0:
k_persist<0,64>, k_persist<1,16>) and the launch-per-op graphs.  The trim keeps every rounding and every summation
tree, so everything is compared bit for bit.

The release library has no read-back of the K/V cache (debug_read is a development hook), so the K/V rows that a step
appends are checked through the step at the next position, whose attention reads them in both contexts.
"""
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))

pytestmark = pytest.mark.gpu


def _engine(tts, tok, persist, roles=True, **kw):
    """persist=False: the launch-per-op graphs (the code predictor's attention as its own k_attn launch); roles=False:
    the all-role persistent kernels"""
    import q3t
    env = {"Q3T_PERSIST": "1" if persist else "0", "Q3T_CP_FUSED_ATTN": "1" if persist else "0",
           "Q3T_TK_ROLES": "1" if roles else "0", "Q3T_CP_ROLES": "1" if roles else "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return q3t.Engine(tts, tok, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    tts, _ = synth_dir("full")
    er = _engine(tts, None, True, max_slots=1, max_ctx=160)                # k_tk_roles + k_cp_roles
    ea = _engine(tts, None, True, roles=False, max_slots=1, max_ctx=160)   # k_persist<0,64> + k_persist<1,16>
    eg = _engine(tts, None, False, max_slots=1, max_ctx=160)               # launch per op
    # a silent fallback cannot pass: the role kernels must be the ones in use, and stay in use
    assert er.persist_status() == 0 and er.persist_kernels() & 5 == 5, (er.persist_status(), er.persist_kernels())
    assert ea.persist_status() == 0 and ea.persist_kernels() == 2 | 8, ea.persist_kernels()
    assert eg.persist_status() == -1
    yield er, ea, eg
    for e in (er, ea, eg):
        e.close()


@pytest.mark.parametrize("case", ["greedy", "sampled", "sampled_speaker"])
def test_generate_72_frames_bit_identical(engines, case):
    """72 frames after the 16-token prompt: the decode crosses KV position 64, where the talker goes from one attention
    split to two"""
    er, ea, eg = engines
    H = er.cfg["hidden"]
    kw = dict(max_len=72, temperature=0.0 if case == "greedy" else 0.9, top_k=50, seed=17, force_frames=72)
    if case == "sampled_speaker":
        kw["speakers"] = [(np.random.default_rng(3).standard_normal(H) * 0.1).astype(np.float32)]
    toks = prompt("full")
    cr = er.generate([toks], **kw)[0]
    ca = ea.generate([toks], **kw)[0]
    cg = eg.generate([toks], **kw)[0]
    assert cr.shape == ca.shape == cg.shape == (72, 16)
    assert np.array_equal(cr, ca), ("all-role kernels", int(np.argmax(np.any(cr != ca, axis=1))))
    assert np.array_equal(cr, cg), ("launch per op", int(np.argmax(np.any(cr != cg, axis=1))))
    assert er.persist_kernels() & 5 == 5 and er.persist_status() == 0


def test_alternating_stage_launches_bit_identical(engines):
    """40 launches, talker step and code-predictor frame in turn, at positions 15, 63 (the last of one split), 64 (the
    first of two) and 130 (three): hidden state, logits and codes against the per-op engine, and the appended K/V rows
    through one more step at the next position"""
    er, _, eg = engines
    H = er.cfg["hidden"]
    rng = np.random.default_rng(29)
    for pos in (15, 63, 64, 130):
        for k in range(5):
            e = (rng.standard_normal(H) * 0.5).astype(np.float32)
            hr, lr = er.talker_forward(e[None], [pos])
            hg, lg = eg.talker_forward(e[None], [pos])
            assert np.array_equal(hr.view(np.uint32), hg.view(np.uint32)), (pos, k)
            assert np.array_equal(lr.view(np.uint32), lg.view(np.uint32)), (pos, k)
            cb0 = int(np.argmax(lr[0, :2048]))
            t = 0.0 if k % 2 == 0 else 0.9
            cr = er.codepred_frame(hr, [cb0], temperature=t, top_k=50, seed=7, frame=k)
            cg = eg.codepred_frame(hg, [cb0], temperature=t, top_k=50, seed=7, frame=k)
            assert np.array_equal(cr, cg), (pos, k, cr, cg)
        e = (rng.standard_normal(H) * 0.5).astype(np.float32)
        hr, lr = er.talker_forward(e[None], [pos + 1])   # reads the K/V row appended at pos
        hg, lg = eg.talker_forward(e[None], [pos + 1])
        assert np.array_equal(hr.view(np.uint32), hg.view(np.uint32)), ("kv", pos)
        assert np.array_equal(lr.view(np.uint32), lg.view(np.uint32)), ("kv", pos)
    assert er.persist_kernels() & 5 == 5 and er.persist_status() == 0


@pytest.mark.parametrize("case", ["1e-3", "1", "1e3", "outlier"])
def test_cp_frame_partial_sums_of_different_magnitude(engines, case):
    """code-predictor frames whose hidden state is scaled by 1e-3, 1 and 1e3, and one with a single 1e4 element: the
    RMSNorm sums of squares then add partial sums of very different magnitude, in an order that must stay the
    per-op GEMV prologue's -- against both untouched paths, greedy and sampled"""
    er, ea, eg = engines
    H = er.cfg["hidden"]
    hid = (np.random.default_rng(41).standard_normal(H) * 1.5).astype(np.float32)
    if case == "outlier":
        hid[517] = 1e4
    else:
        hid *= np.float32(float(case))
    for frame, t in ((0, 0.0), (1, 0.9)):
        # (the codes only: a frame asked for its logits runs launch per op in every context)
        cr = er.codepred_frame(hid[None], [123], temperature=t, top_k=50, seed=5, frame=frame)
        ca = ea.codepred_frame(hid[None], [123], temperature=t, top_k=50, seed=5, frame=frame)
        cg = eg.codepred_frame(hid[None], [123], temperature=t, top_k=50, seed=5, frame=frame)
        assert np.array_equal(cr, ca) and np.array_equal(cr, cg), (case, t, cr, ca, cg)
    assert er.persist_kernels() & 5 == 5 and er.persist_status() == 0
