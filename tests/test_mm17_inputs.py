"""CPU check of the inputs tests/test_gpu_mm17.py feeds its greedy code-predictor case (tests/mm17_inputs.py): the cap
on near-tie decisions there is only meaningful if the oracle's own decisions on these inputs are rarely near-ties.
With the chosen seed, at most CP_MAX_TIE_FRAC of the oracle's greedy decisions have a top-2 logit gap below twice the
tie tolerance, for every slot count the GPU test runs."""
import pytest

from mm17_inputs import CP_MAX_TIE_FRAC, CP_SEED, CP_SLOTS, CP_TIE_TOL, cp_frame_inputs, oracle_tie_share
from oracle_py import Oracle
from q3t_testutil import synth_dir


@pytest.fixture(scope="module")
def orc():
    o = Oracle(*synth_dir("wide17"))
    yield o
    o.close()


def test_wide17_has_the_17_layout(orc):
    c = orc.cfg
    assert (c["hidden"], c["inter"], c["n_heads"], c["n_kv"], c["head_dim"], c["n_layers"]) == (2048, 6144, 16, 8, 128, 2)
    assert (c["cp_hidden"], c["cp_inter"], c["cp_heads"], c["cp_kv"], c["cp_layers"], c["has_mtp"]) == (1024, 3072, 16, 8, 2, 1)
    assert (c["text_vocab"], c["text_dim"], c["codec_vocab"], c["cp_vocab"]) == (1024, 128, 3072, 2048)
    assert (c["tts_bos"], c["tts_eos"], c["tts_pad"]) == (1001, 1002, 1000)


def test_inputs_are_shared_prefixes():
    hid, cb0 = cp_frame_inputs(2048)
    assert hid.shape == (CP_SLOTS[-1], 2048) and cb0.shape == (CP_SLOTS[-1],)
    h4, c4 = cp_frame_inputs(2048, n=CP_SLOTS[-1], seed=CP_SEED)
    assert (h4 == hid).all() and (c4 == cb0).all()
    assert 0 <= cb0.min() and cb0.max() < 2048


@pytest.mark.parametrize("slots", CP_SLOTS)
def test_oracle_decisions_are_rarely_near_ties(orc, slots):
    share = oracle_tie_share(orc, slots)
    print(f"wide17 greedy code-predictor inputs, {slots} slots: {share:.4f} of the oracle's decisions within {2 * CP_TIE_TOL}")
    assert share <= CP_MAX_TIE_FRAC, (slots, share)
