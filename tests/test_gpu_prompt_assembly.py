"""The prompt assembly shared by q3t_prefill_embd, generate() and the admissions of generate_queue()
(Engine::assemble_prompts), where the other suites leave it untested: nonzero speaker rows that differ per utterance,
the nothink prompt (language_id -1: no language row, one prompt row shorter), and the argument errors.

  oracle      prefill / trailing / pad rows against the CPU oracle for both prompts, with and without a speaker row
              (the tolerances of test_gpu_parity.py); a language id at or above codec_vocab is rejected
  first wave  test_gpu_queue.py's first-wave test with a distinct speaker per utterance, for both prompts: the queue's
              admissions assemble what generate() assembles, bit for bit; speakers for only some utterances are
              rejected
  1.7B        the code-predictor passes of a model with mtp_proj stage their gathered rows in cp_in1_, the main
              stream's speaker scratch: an admission that overlaps the frame loop keeps its speaker rows in its own
              scratch, so a queue with 4 utterances in flight equals the same queue with 1 in flight
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle_py import Oracle
from q3t_testutil import REPO, prompt, rel_err, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu
TOL = {"tiny": 3e-3, "full": 5e-3}   # test_gpu_parity.py's


def _speakers(n, H):
    rng = np.random.default_rng(2)
    return [(rng.standard_normal(H) * 0.02).astype(np.float32) for _ in range(n)]


@pytest.mark.parametrize("cfg", ["tiny", "full"])
def test_prefill_rows_match_oracle_for_both_prompts(cfg):
    import q3t
    tts, tok = synth_dir(cfg)
    eng = q3t.Engine(tts, None, device=0, max_slots=4, max_ctx=128)
    orc = Oracle(tts, tok)
    try:
        toks = prompt(cfg)
        spk = _speakers(1, eng.cfg["hidden"])[0]
        for lang in (2050, -1):
            for sp in (None, spk):
                pg, tg, padg = eng.prefill_embd(toks, sp, language_id=lang)
                po, to, pado = orc.prefill_embd(toks, sp, language_id=lang)
                assert pg.shape == po.shape and tg.shape == to.shape
                assert len(pg) == (9 if lang >= 0 else 8) + (sp is not None)
                assert rel_err(pg, po) < TOL[cfg] and rel_err(tg, to) < TOL[cfg] and rel_err(padg, pado) < TOL[cfg]
        for lang in (eng.cfg["codec_vocab"], eng.cfg["codec_vocab"] + 1000):
            with pytest.raises(q3t.Q3TError, match="language id out of range"):
                eng.prefill_embd(toks, spk, language_id=lang)
    finally:
        eng.close()
        orc.close()


def _queue_prompts(n, seed):   # test_gpu_queue.py's: 5..12 text tokens, so EOS stops fall inside max_len
    base = prompt("full")
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(5, 13))
        tail = [(t + 13 * i) % 900 + 20 for t in base[4:]]
        out.append(base[:4] + tail[:k - 4])
    return out


@pytest.mark.parametrize("language_id", [2050, -1])
def test_queue_first_wave_equals_generate_with_speakers(language_id):
    import q3t
    tts, tok = synth_dir("full")
    nf, slots, n_utt = 24, 4, 8
    eng = q3t.Engine(tts, None, device=0, max_slots=slots, max_ctx=nf + 40)
    try:
        prompts = _queue_prompts(n_utt, 11)
        spk = _speakers(n_utt, eng.cfg["hidden"])
        assert all(np.any(s != 0) for s in spk) and not np.array_equal(spk[0], spk[1])
        kw = dict(max_len=nf, temperature=0.9, top_k=50, seed=31, language_id=language_id)
        q = eng.generate_queue(prompts, speakers=spk, **kw)
        g = eng.generate(prompts[:slots], speakers=spk[:slots], **kw)
        for u in range(slots):
            assert np.array_equal(q[u], g[u]), (u, len(q[u]), len(g[u]))
        # generate() after a queue run keys sampling by slot again
        assert all(np.array_equal(a, b) for a, b in zip(eng.generate(prompts[:slots], speakers=spk[:slots], **kw), g))
        # speakers for only some utterances (null rows, which the Python wrapper cannot express: straight through the
        # C ABI), missing after the first row and missing in the first row
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n_utt)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        p = q3t.default_params(**kw)
        codes, n_fr = np.zeros((n_utt, nf, 16), np.int32), np.zeros(n_utt, np.int32)
        for missing in (n_utt - 1, 0):
            rows = [None if u == missing else s.ctypes.data_as(C.POINTER(C.c_float)) for u, s in enumerate(spk)]
            sarr = (C.POINTER(C.c_float) * n_utt)(*rows)
            with pytest.raises(q3t.Q3TError, match="speaker embedding must be given for all or none of the utterances"):
                q3t._check(q3t.lib().q3t_generate_queue(eng.h, n_utt, tarr, ntok, sarr, C.byref(p), codes, n_fr, 0))
    finally:
        eng.close()


def test_queue_on_the_17_layout_is_admission_invariant_with_speakers():
    import q3t
    tts, tok = synth_dir("tiny17")
    eng = q3t.Engine(tts, None, device=0, max_slots=4, max_ctx=96)
    try:
        base = prompt("tiny17")
        n_utt = 8
        prompts = [base[:4] + [(t + 37 * i) % 900 + 20 for t in base[4:]] for i in range(n_utt)]
        kw = dict(speakers=_speakers(n_utt, eng.cfg["hidden"]), max_len=24, temperature=0.9, top_k=50, seed=31)
        a = eng.generate_queue(prompts, max_active=4, **kw)
        b = eng.generate_queue(prompts, max_active=1, **kw)
        assert all(0 < len(c) <= 24 for c in a)
        for u in range(n_utt):
            assert np.array_equal(a[u], b[u]), (u, len(a[u]), len(b[u]))
    finally:
        eng.close()
