"""The paired pass of the one-slot code-predictor frame (persist_cp.hip k_cp_roles, Q3T_CP_PAIR): passes 0 and 1 run as
two interleaved chains through the same role workgroups, each chain on its own set of hand-off vectors.

Pass 1 reads pass 0's K/V rows of every layer, so an ordering or buffer-set mistake shows up as a changed code (or as a
hand-off wait that gives up: persist_status() != 0).  Everything is compared BIT-EXACT against the launch-per-op graphs
with the code predictor's attention as its own launch, whose arithmetic the persistent frame reproduces bit for bit.
The kernel exists only at the 0.6B code-predictor shapes (synth "full"), so there is no smaller shape to use; a frame is
about 1 ms persistent and a few ms per-op.
"""
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, prompt, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))

pytestmark = pytest.mark.gpu

# (temperature, top_k): greedy, the bench's sampling, and a wide one -- temperature 1.5 / top-k 1000 goes through the
# selection's general path in both engines and puts most logits into the cumulative sum, so a last-bit difference in
# pass 0's K/V rows is far more likely to move a code than at top-k 50
SETTINGS = [(0.0, 50), (0.9, 50), (1.5, 1000)]
SCALES = (0.1, 1.5, 8.0)
FRAMES_PER_SCALE = 24   # x 3 scales x 3 settings = 216 frames


def _engine(tts, tok, persist, **kw):
    """persist=False: the launch-per-op graphs with the code predictor's attention as its own k_attn launch"""
    import q3t
    env = {"Q3T_PERSIST": "1" if persist else "0", "Q3T_CP_FUSED_ATTN": "1" if persist else "0",
           "Q3T_TK_ROLES": "1", "Q3T_CP_ROLES": "1"}
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
    tts, tok = synth_dir("full")
    ep = _engine(tts, tok, True, max_slots=1, max_ctx=96)
    eg = _engine(tts, tok, False, max_slots=1, max_ctx=96)
    assert eg.persist_status() == -1
    yield ep, eg
    ep.close()
    eg.close()


@pytest.fixture(autouse=True)
def _roles_kernel_in_use(engines):
    ep, _ = engines
    assert ep.persist_status() == 0
    assert ep.persist_kernels() & 4, ep.persist_kernels()   # k_cp_roles
    yield
    assert ep.persist_status() == 0, "a hand-off wait gave up"


@pytest.mark.parametrize("temperature,top_k", SETTINGS)
def test_codes_bit_identical_over_many_frames(engines, temperature, top_k):
    ep, eg = engines
    H = ep.cfg["hidden"]
    rng = np.random.default_rng(101 + top_k)
    bad = []
    frame = 0
    for scale in SCALES:
        cb0s = [0, 2047] + [int(c) for c in rng.integers(0, 2048, FRAMES_PER_SCALE - 2)]
        for cb0 in cb0s:
            hid = (rng.standard_normal(H) * scale).astype(np.float32)
            kw = dict(temperature=temperature, top_k=top_k, seed=7, frame=frame)
            cp = ep.codepred_frame(hid[None], [cb0], **kw)
            cg = eg.codepred_frame(hid[None], [cb0], **kw)
            assert cp.shape == cg.shape == (1, 15)
            if not np.array_equal(cp, cg):
                bad.append((scale, cb0, frame, int(np.argmax(cp[0] != cg[0]))))
            frame += 1
    assert frame == len(SCALES) * FRAMES_PER_SCALE
    assert not bad, (len(bad), bad[:8])


def test_alternating_inputs_no_stale_match(engines):
    """X, Y, X, Y, ... back to back on the same engines: a granule left by the previous launch in either buffer set
    carries the other input's payload, so a stale match changes a code"""
    ep, eg = engines
    H = ep.cfg["hidden"]
    rng = np.random.default_rng(77)
    inputs = [((rng.standard_normal(H) * 1.5).astype(np.float32), 5), ((rng.standard_normal(H) * 1.5).astype(np.float32), 1900)]
    kw = dict(temperature=0.9, top_k=50, seed=11, frame=3)
    want = [eg.codepred_frame(h[None], [c], **kw) for h, c in inputs]
    assert not np.array_equal(want[0], want[1])
    for n in range(40):
        h, c = inputs[n & 1]
        got = ep.codepred_frame(h[None], [c], **kw)
        assert np.array_equal(got, want[n & 1]), (n, got, want[n & 1])


def test_generate_bit_exact(engines):
    """48 frames end to end: the frame graphs replay the talker and code-predictor launches alternately"""
    ep, eg = engines
    toks = prompt("full")
    spk = np.zeros(ep.cfg["hidden"], np.float32)
    kw = dict(speakers=[spk], max_len=48, temperature=0.9, top_k=50, seed=9, force_frames=48)
    cp = ep.generate([toks], **kw)[0]
    cg = eg.generate([toks], **kw)[0]
    assert cp.shape == cg.shape == (48, 16)
    assert np.array_equal(cp, cg), int(np.argmax(np.any(cp != cg, axis=1)))
