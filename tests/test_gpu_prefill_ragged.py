"""The ragged causal prefill (q3t_talker_prefill_ragged): prompts of different lengths packed into one pass, the form
the per-utterance entry points run (Engine::prefill_ragged; k_prefill_attn takes each utterance's first row and row count
from device arrays).

Row i of utterance u must be, bit for bit, what q3t_talker_prefill computes for that utterance alone at its length:
the hidden rows, the last row's logits, and the K/V rows it writes -- read back by one decode step at position
n_rows[u] on the utterance's slot.  The decode step compares like with like only on the same slot and slot count, so
the list is rotated: each utterance takes slot 0 in turn and is compared with its own single prefill into slot 0.
Lengths [1, 10, 8, 9] (the shortest and the longest a prompt can be, and the 8 / 9 / 10 rows of real prompts) and [10]
alone; kernel families of a 1-slot and a 4-slot step; the 0.6B and the 1.7B layout.  Equal lengths [9, 9, 9, 9] equal
the uniform entry point called once with four utterances.
"""
import os
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["full", "tiny17"])
def eng(request):
    import q3t
    tts, _ = synth_dir(request.param)
    e = q3t.Engine(tts, None, device=0, max_slots=4, max_ctx=64)
    yield e
    e.close()


def _rows(H, lens, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, H)) * 0.5).astype(np.float32) for n in lens]


def _step(eng, family, pos0, x):
    """one decode step of `family` slots; slot 0 at pos0 reads the K/V rows [0, pos0) the prefill wrote there"""
    pos = np.zeros(family, np.int32)
    pos[0] = pos0
    h, lg = eng.talker_forward(np.repeat(x[None], family, axis=0), pos)
    return h[0], lg[0]


@pytest.mark.parametrize("family", [1, 4])
@pytest.mark.parametrize("lens", [[1, 10, 8, 9], [10]])
def test_ragged_rows_equal_the_single_prefill(eng, family, lens):
    H = eng.cfg["hidden"]
    rows = _rows(H, lens, 40 + len(lens))
    x = _rows(H, [1], 7)[0][0]
    ref = []   # each utterance alone, into slot 0
    for r in rows:
        hid, lg = eng.talker_prefill(r[None], family_slots=family)
        ref.append((hid[0], lg[0]) + _step(eng, family, len(r), x))
    for rot in range(len(lens)):
        order = [(rot + j) % len(lens) for j in range(len(lens))]
        hid, lg = eng.talker_prefill_ragged([rows[u] for u in order], family_slots=family)
        for j, u in enumerate(order):
            assert hid[j].shape == ref[u][0].shape
            assert np.array_equal(hid[j], ref[u][0]), (rot, u, float(np.abs(hid[j] - ref[u][0]).max()))
            assert np.array_equal(lg[j], ref[u][1]), (rot, u, float(np.abs(lg[j] - ref[u][1]).max()))
        hs, ls = _step(eng, family, lens[rot], x)   # slot 0 holds utterance `rot`
        assert np.array_equal(hs, ref[rot][2]) and np.array_equal(ls, ref[rot][3]), (rot, float(np.abs(ls - ref[rot][3]).max()))


@pytest.mark.parametrize("family", [1, 4])
def test_equal_lengths_equal_the_uniform_entry_point(eng, family):
    H = eng.cfg["hidden"]
    rows = _rows(H, [9, 9, 9, 9], 3)
    x = _rows(H, [4], 8)[0]
    pos = np.full(4, 9, np.int32)
    hu, lu = eng.talker_prefill(np.stack(rows), family_slots=family)
    su = eng.talker_forward(x, pos)
    hr, lr = eng.talker_prefill_ragged(rows, family_slots=family)
    sr = eng.talker_forward(x, pos)
    assert np.array_equal(np.stack(hr), hu) and np.array_equal(lr, lu)
    assert np.array_equal(sr[0], su[0]) and np.array_equal(sr[1], su[1])


def test_ragged_argument_errors(eng):
    import q3t
    H = eng.cfg["hidden"]
    for lens in ([11], [3, 0, 2]):
        with pytest.raises(q3t.Q3TError, match="prefill rows must be in"):
            n_rows = np.array(lens, np.int32)
            q3t._check(q3t.lib().q3t_talker_prefill_ragged(eng.h, len(lens), n_rows, np.zeros(40 * H, np.float32), 0, None, None))
    with pytest.raises(q3t.Q3TError, match="bad utterance count"):
        eng.talker_prefill_ragged(_rows(H, [2] * 5, 1))
