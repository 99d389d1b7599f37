"""conv()'s kernel choice (q3t::conv_kernel, host arithmetic: runs without a GPU) at the decoder's shapes and at the
shapes tests/test_gpu_voc_ops.py relies on, with the Q3T_CONV_* switches."""
import pytest

from voc_ops_lib import GENERIC, MT, PD, ConvDesc, load


@pytest.fixture(scope="module")
def ops():
    return load()


def desc(C_in, C_out, k, M, nb=1, dil=1, xh=True, ct=None, y=True):
    d = ConvDesc()
    d.T_in, d.C_in, d.C_out, d.nb, d.xbs, d.ybs = M, C_in, C_out, nb, M, M
    if xh:
        d.xh = 4096      # (never dereferenced: only null or not)
    else:
        d.x = 4096
    if y:
        d.y = 4096
    d.w = d.ct_w = 4096
    if ct:
        d.ct_k, d.ct_st, d.ct_trim = ct
        d.T_out = (M - 1) * ct[1] + ct[0] - 2 * ct[2]
        d.ybs = d.T_out
    else:
        d.M, d.n_taps, d.dil, d.pad, d.so = M, k, dil, (k - 1) * dil, 1
    return d


BIG = 255 * 256 + 1      # the fewest rows with 512 256-row tiles at two channel tiles
BIG1 = 511 * 256 + 1     # ... at one

CASES = [
    # (descriptor arguments, environment, expected (family, RB, NT, TW or TAPS, MINB, xcd))
    (dict(C_in=96, C_out=96, k=7, M=300, nb=3, dil=9), {}, (MT, 1, 96, 7, 2, 1)),
    (dict(C_in=32, C_out=128, k=3, M=129), {}, (MT, 1, 64, 3, 2, 1)),
    (dict(C_in=96, C_out=192, k=1, M=1), {}, (MT, 1, 96, 1, 2, 1)),
    (dict(C_in=96, C_out=96, k=1, M=BIG1), {}, (MT, 1, 96, 1, 3, 1)),
    (dict(C_in=192, C_out=192, k=1, M=BIG), {}, (MT, 1, 96, 1, 3, 1)),
    (dict(C_in=192, C_out=192, k=1, M=BIG - 1), {}, (MT, 1, 96, 1, 2, 1)),
    (dict(C_in=384, C_out=384, k=1, M=BIG), {}, (MT, 2, 96, 1, 2, 1)),
    (dict(C_in=192, C_out=192, k=7, M=BIG, dil=3), {}, (PD, 4, 96, 7, 1, 1)),
    (dict(C_in=192, C_out=128, k=7, M=BIG, dil=9), {}, (PD, 4, 64, 7, 1, 1)),
    (dict(C_in=192, C_out=192, k=7, M=BIG), {"Q3T_CONV_PD": "1"}, (PD, 2, 96, 7, 1, 1)),
    (dict(C_in=192, C_out=192, k=7, M=BIG), {"Q3T_CONV_PD": "0"}, (MT, 2, 96, 7, 2, 1)),
    (dict(C_in=128, C_out=128, k=7, M=BIG), {"Q3T_CONV_PD": "0"}, (MT, 2, 64, 7, 2, 1)),
    (dict(C_in=192, C_out=192, k=7, M=BIG), {"Q3T_CONV_XCD": "0"}, (PD, 4, 96, 7, 1, 0)),
    (dict(C_in=96, C_out=96, k=7, M=BIG1), {}, (MT, 2, 96, 7, 2, 1)),                       # below Q3T_CONV_PD_MINC
    (dict(C_in=96, C_out=96, k=7, M=BIG1), {"Q3T_CONV_PD_MINC": "96"}, (PD, 4, 96, 7, 1, 1)),
    (dict(C_in=192, C_out=192, k=7, M=BIG - 1), {}, (MT, 1, 96, 7, 2, 1)),
    (dict(C_in=192, C_out=96, k=0, M=129, nb=3, ct=(6, 3, 3)), {}, (MT, 1, 96, 3, 2, 1)),
    (dict(C_in=1536, C_out=768, k=0, M=2051, ct=(16, 8, 8)), {}, (PD, 4, 96, 2, 1, 1)),
    (dict(C_in=1536, C_out=768, k=0, M=2051, ct=(16, 8, 8)), {"Q3T_CONV_PD_CT": "0"}, (MT, 2, 96, 3, 2, 1)),
    (dict(C_in=768, C_out=384, k=0, M=6479, ct=(10, 5, 5)), {}, (PD, 4, 96, 2, 1, 1)),
    (dict(C_in=768, C_out=384, k=0, M=6479 - 256, ct=(10, 5, 5)), {}, (MT, 1, 96, 3, 2, 1)),
    (dict(C_in=384, C_out=192, k=0, M=BIG, ct=(8, 4, 4)), {}, (MT, 2, 96, 3, 2, 1)),            # C_in below 768
    (dict(C_in=20, C_out=40, k=3, M=65, xh=False), {}, (GENERIC, 0, 0, 0, 0, 0)),
    (dict(C_in=96, C_out=1, k=7, M=65), {}, (GENERIC, 0, 0, 0, 0, 0)),
    (dict(C_in=100, C_out=96, k=1, M=65), {}, (GENERIC, 0, 0, 0, 0, 0)),
    (dict(C_in=96, C_out=96, k=1, M=0), {}, (0, 0, 0, 0, 0, 0)),
    (dict(C_in=96, C_out=96, k=1, M=65, y=False), {}, (0, 0, 0, 0, 0, 0)),                      # no output: an error
    (dict(C_in=192, C_out=96, k=0, M=1, ct=(6, 3, 3)), {}, (0, 0, 0, 0, 0, 0)),                 # T_out = 0
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_conv_kernel_choice(ops, monkeypatch, i):
    args, env, want = CASES[i]
    for k in ("Q3T_CONV_PD", "Q3T_CONV_PD_CT", "Q3T_CONV_PD_MINC", "Q3T_CONV_XCD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert ops.kernel(desc(**args)) == want
