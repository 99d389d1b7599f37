"""Inputs shared by tests/test_gpu_mm17.py and tests/test_mm17_inputs.py: the code-predictor frames of the wide17
model (tools/q3t_synth.c) whose greedy codes the GPU test compares with the oracle's.

The GPU test lets a greedy code differ from the oracle's argmax when the oracle's own logit gap to it is below
CP_TIE_TOL, for at most CP_MAX_TIE_FRAC of the decisions.  That cap only means something if the oracle's decisions on
these inputs are not near-ties to begin with, so CP_SEED was chosen on the CPU (tests/test_mm17_inputs.py asserts it)
such that at most CP_MAX_TIE_FRAC of the oracle's own greedy decisions have a top-2 gap below 2 * CP_TIE_TOL, over
the first CP_SLOTS[0] slots and over all CP_SLOTS[1] of them."""
import numpy as np

CP_SEED = 82
CP_SLOTS = (4, 33)       # one 32-token tile; one token in the second tile
CP_TIE_TOL = 5e-2        # logit gap within which a greedy code may differ from the oracle's argmax
CP_MAX_TIE_FRAC = 0.05   # share of the greedy decisions that may take that branch


def cp_frame_inputs(hidden, n=CP_SLOTS[-1], seed=CP_SEED):
    """(talker hidden states [n][hidden] f32, CB0 codes [n] i32); the first k rows are the inputs of a k-slot case"""
    rng = np.random.default_rng(seed)
    hid = (rng.standard_normal((n, hidden)) * 1.5).astype(np.float32)
    cb0 = rng.integers(0, 2048, n).astype(np.int32)
    return hid, cb0


def oracle_tie_share(orc, n, seed=CP_SEED):
    """share of the oracle's own greedy decisions over the first n slots whose top-2 logit gap is below 2 * CP_TIE_TOL"""
    hid, cb0 = cp_frame_inputs(orc.cfg["hidden"], seed=seed)
    close = total = 0
    for s in range(n):
        _, lg = orc.cp_frame(hid[s], int(cb0[s]), want_logits=True)
        top2 = np.sort(lg, axis=1)[:, -2:]
        close += int(((top2[:, 1] - top2[:, 0]) < 2 * CP_TIE_TOL).sum())
        total += lg.shape[0]
    return close / total
