"""The layers above the vocoder stream's C ABI: qwen3-tts-cli --stream-full (generation through the frame callback,
each delivery pushed into a vocoder stream) writes the WAV of the same command without the flag, byte for byte; and the
C++ mirror's AudioTokenizerDecoder::stream_* (tests/cpp/test_voc_stream_api.cpp) returns the samples of the ctypes path."""
import os
import subprocess
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu
CLI = os.path.join(REPO, "qwen3-tts-jetson_amd", "cpp", "qwen3-tts-cli")
BIN = os.path.join(REPO, "tests", "cpp", "_build", "test_voc_stream_api")
# the synthetic model of every CLI test (tests/test_pipeline.py, tests/test_boundary.py): the CLI tokenizes real text,
# whose template ids lie outside the tiny model's 1,024-entry text vocabulary ("text token out of range")
CLI_CFG = "full"


def _model_dir(tmp_path):
    tts, tok = synth_dir(CLI_CFG)
    d = tmp_path / "models"   # no chunked engine file: the whole-utterance vocoder
    d.mkdir()
    os.symlink(tts, d / "qwen3-tts-0.6b-f16.gguf")
    os.symlink(tok, d / "qwen3-tts-tokenizer-f16.gguf")
    return str(d)


def test_cli_stream_full_writes_the_same_wav(tmp_path):
    assert os.path.exists(CLI), "qwen3-tts-cli missing: run __graft_entry__.build()"
    d = _model_dir(tmp_path)
    wavs = []
    for name, extra in (("plain.wav", []), ("stream.wav", ["--stream-full", "7"])):
        out = str(tmp_path / name)
        r = subprocess.run([CLI, "-m", d, "-t", "Hello. This is a test.", "-o", out, "--max-tokens", "40",
                            "--temperature", "0.9", "--seed", "5"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(out, "rb") as f:
            wavs.append(f.read())
    assert len(wavs[0]) > 44 + 2 * 1000, "the plain run wrote (almost) no audio"
    assert wavs[0] == wavs[1]
    assert np.abs(np.frombuffer(wavs[0][44:], np.int16)).max() > 0


@pytest.mark.parametrize("cfg", ["tiny", "full"])
def test_cpp_stream_methods_match_ctypes_path(tmp_path, cfg):
    import q3t
    assert os.path.exists(BIN), "tests/cpp/_build/test_voc_stream_api missing: run __graft_entry__.build()"
    _, tok = synth_dir(cfg)
    codes = np.random.default_rng(21).integers(0, 2048, size=(45, 16), dtype=np.int32)
    codes.tofile(tmp_path / "voc_codes.bin")
    r = subprocess.run([BIN, tok, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout, (r.returncode, r.stdout, r.stderr[-3000:])
    got = np.fromfile(tmp_path / "voc_stream.bin", np.float32)
    eng = q3t.Engine(None, tok, device=0)
    try:
        want = eng.vocoder(codes, 0)
        with eng.vocoder_stream(max_frames=45) as st:
            mine = np.concatenate([st.push(codes[:20]), st.push(codes[20:])])
    finally:
        eng.close()
    assert np.array_equal(mine, want)
    assert np.array_equal(got, want)
