"""CPU tests (no GPU) of the per-utterance parameter ABI (include/q3t_backend.h: q3t_utt_params, q3t_utt_params_from,
q3t_generate_utt, q3t_generate_queue_utt, q3t_talker_prefill_ragged): the symbols are exported, the record's layout is
the one the Python wrapper declares, q3t_gen_params kept its layout, and q3t_utt_params_from copies the call-wide values
field for field.  The wrapper's per_utt plumbing (overrides, unknown keys, optional speakers) is host code as well."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from q3t_testutil import REPO

PKG = os.path.join(REPO, "qwen3-tts-jetson_amd")
sys.path.insert(0, PKG)

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "q3t_backend.h"
#define F(s, f) printf(#s "." #f " %zu\n", offsetof(s, f))
int main(void) {
    printf("q3t_gen_params %zu\n", sizeof(q3t_gen_params));
    F(q3t_gen_params, max_len); F(q3t_gen_params, language_id); F(q3t_gen_params, repetition_penalty);
    F(q3t_gen_params, temperature); F(q3t_gen_params, top_k); F(q3t_gen_params, seed); F(q3t_gen_params, force_frames);
    printf("q3t_utt_params %zu\n", sizeof(q3t_utt_params));
    F(q3t_utt_params, language_id); F(q3t_utt_params, max_len); F(q3t_utt_params, repetition_penalty);
    F(q3t_utt_params, temperature); F(q3t_utt_params, top_k); F(q3t_utt_params, force_frames);
    return 0;
}
"""


def test_new_symbols_are_exported():
    import q3t
    lib = C.CDLL(q3t.LIB_PATH)
    for name in ("q3t_utt_params_from", "q3t_generate_utt", "q3t_generate_queue_utt", "q3t_talker_prefill_ragged"):
        assert hasattr(lib, name), name
        assert name in q3t.EXPORTS, name


def test_struct_layouts(tmp_path):
    import q3t
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    # q3t_gen_params is what it was before the per-utterance records existed: 40 bytes, the seed 8-aligned at 24
    assert int(out["q3t_gen_params"]) == 40 == C.sizeof(q3t.GenParams)
    assert [int(out[f"q3t_gen_params.{f}"]) for f in ("max_len", "language_id", "repetition_penalty", "temperature", "top_k",
                                                     "seed", "force_frames")] == [0, 4, 8, 12, 16, 24, 32]
    for name, _ in q3t.GenParams._fields_:
        assert int(out[f"q3t_gen_params.{name}"]) == getattr(q3t.GenParams, name).offset, name
    assert int(out["q3t_utt_params"]) == 24 == C.sizeof(q3t.UttParams)
    for name, _ in q3t.UttParams._fields_:
        assert int(out[f"q3t_utt_params.{name}"]) == getattr(q3t.UttParams, name).offset, name


def test_utt_params_from_copies_the_call_wide_values():
    import q3t
    p = q3t.default_params()
    up = q3t.UttParams()
    q3t.lib().q3t_utt_params_from(C.byref(p), C.byref(up))
    assert (up.language_id, up.max_len, up.top_k, up.force_frames) == (2050, 4096, 50, 0)
    assert up.repetition_penalty == np.float32(1.05) and up.temperature == np.float32(0.9)
    p = q3t.default_params(max_len=17, language_id=-1, repetition_penalty=1.5, temperature=0.0, top_k=3, seed=99, force_frames=5)
    q3t.lib().q3t_utt_params_from(C.byref(p), C.byref(up))
    assert (up.language_id, up.max_len, up.repetition_penalty, up.temperature, up.top_k, up.force_frames) == (-1, 17, 1.5, 0.0, 3, 5)
    q3t.lib().q3t_utt_params_from(None, C.byref(up))   # null arguments: no effect
    q3t.lib().q3t_utt_params_from(C.byref(p), None)
    assert up.max_len == 17


def test_wrapper_builds_the_records():
    import q3t
    p = q3t.default_params(max_len=24, temperature=0.5)
    up = q3t.utt_params(p, [None, dict(temperature=0.0, max_len=5), dict(language_id=-1, top_k=8, repetition_penalty=1.2)], 3)
    assert [(r.language_id, r.max_len, r.top_k) for r in up] == [(2050, 24, 50), (2050, 5, 50), (-1, 24, 8)]
    assert [r.temperature for r in up] == [0.5, 0.0, 0.5]
    assert up[2].repetition_penalty == np.float32(1.2) and up[0].repetition_penalty == np.float32(1.05)
    with pytest.raises(ValueError, match="unknown key 'seed'"):
        q3t.utt_params(p, [dict(seed=1)], 1)
    with pytest.raises(ValueError, match="one entry"):
        q3t.utt_params(p, [None], 2)
    # speakers: None entries only where the call is per utterance
    H = 8
    arr, keep = q3t._speaker_array([np.ones(H, np.float32), None], 2, True)
    assert bool(arr[0]) and not bool(arr[1]) and keep[1] is None
    with pytest.raises(ValueError, match="only with per_utt"):
        q3t._speaker_array([np.ones(H, np.float32), None], 2, False)


def test_null_context_is_an_error_not_a_crash():
    import q3t
    lib = q3t.lib()
    nf = np.zeros(1, np.int32)
    assert lib.q3t_generate_utt(None, 1, None, nf, None, None, None, nf, nf, None, None, 0) == -1
    assert b"null context" in lib.q3t_last_error()
    assert lib.q3t_generate_queue_utt(None, 1, None, nf, None, None, None, None, nf, 0, None, None, 0) == -1
    assert lib.q3t_talker_prefill_ragged(None, 1, nf, np.zeros(4, np.float32), 0, None, None) == -1
