"""CPU checks of tests/voc_stream_ops_ref.py, the reference and tolerance of tests/test_gpu_voc_stream_ops.py (no GPU):
  * the float32 re-evaluation of the reference in the kernel's summation structure stays inside the tolerance on the
    GPU test's own cases; its worst need (printed) defines C_TOL_STREAM = 4 x that need, the margin
    tests/test_attn_ops_ref.py states for the decode attention;
  * the windowed reference agrees with voc_ops_ref.attention on the whole sequence, so both files describe one operation;
  * mutation checks: a defect the cached attention could have, applied to the reference, moves some output element by
    at least 8 x its tolerance.
"""
import numpy as np
import pytest

import voc_ops_ref as R
import voc_stream_ops_ref as S

U = S.U


def rotated(P, n, nH):
    qkv, rope = S.case(P, n, nH)
    q = S.rope32(qkv[:, 0], rope).astype(np.float64)
    k = S.rope32(qkv[:, 1], rope).astype(np.float64)
    return q, k, qkv[:, 2].astype(np.float64)


@pytest.fixture(scope="module")
def need():
    worst = 0.0
    for P, n in S.CASES:
        for nH in S.HEADS:
            q, k, v = rotated(P, n, nH)
            ref, allow = S.attention_rows(q[P:], k, v, P)
            got = S.eval32(q[P:], k, v, P).astype(np.float64)
            assert np.isfinite(got).all()
            worst = max(worst, R.need_c(got, ref, U * allow))
    return worst


def test_f32_reevaluation_defines_the_constant(need):
    print(f"float32 re-evaluation need {need:.3f} => C_TOL_STREAM >= {4 * need:.3f} (is {S.C_TOL_STREAM})")
    assert 4.0 * need <= S.C_TOL_STREAM * 1.0001, "C_TOL_STREAM is below 4 x the measured need"
    assert S.C_TOL_STREAM <= 4.0 * need * 1.05, "C_TOL_STREAM is not the measured constant"


def test_windowed_reference_is_the_whole_sequence_reference():
    for P, n in ((0, 33), (63, 2), (100, 70)):
        q, k, v = rotated(P, n, 2)
        whole, allow_w = R.attention(q, k, v)
        rows, allow = S.attention_rows(q[P:], k, v, P)
        assert np.allclose(rows, whole[P:], rtol=1e-13, atol=1e-15)
        assert np.allclose(allow, allow_w[P:], rtol=1e-13)


@pytest.mark.parametrize("defect", ["chunk_from_P", "drops_key_P_minus_1", "off_by_one_mask"])
def test_mutations_are_noticed(defect):
    P, n, nH = 63, 2, 2
    q, k, v = rotated(P, n, nH)
    ref, allow = S.attention_rows(q[P:], k, v, P)
    if defect == "chunk_from_P":            # keys before the push ignored
        bad, _ = S.attention_rows(q[P:], k[P:], v[P:], 0)
    elif defect == "drops_key_P_minus_1":   # the last cached row before the push not read
        keep = np.arange(P + n) != P - 1
        kk, vv = k.copy(), v.copy()
        kk[~keep] = 0.0
        vv[~keep] = 0.0
        bad, _ = S.attention_rows(q[P:], kk, vv, P)
    else:                                   # query P + i sees key P + i + 1; the last one a row past P + n
        k2 = np.concatenate([k, k[:1]])
        v2 = np.concatenate([v, 5.0 + v[:1]])
        bad, _ = S.attention_rows(q[P:], k2, v2, P + 1)
    ratio = float(np.max(np.abs(bad - ref) / S.tol(ref, allow)))
    print(f"{defect}: moves an output element by {ratio:.3g} x its tolerance")
    assert ratio >= 8.0
