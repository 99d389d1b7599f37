"""The layers above the open queue: qwen3-tts-cli --serve --queue-open 2 (Qwen3TTS::serve_queue over
q3t_generate_queue_open) on the `full` synthetic model, as test_gpu_queue_stream_cli.py runs --queue.  Five requests of
different lengths and one with a malformed third field are piped at once, with and without --stream-full 4.  There is one
OK line per good request and one ERR line for the bad one, which never enters the queue; every WAV is byte-identical to
the one made from Engine.generate_queue's codes of the good requests, in line order, at two slots, through
Engine.vocoder(); the exit status after `quit` is 0.

That a request which arrives late is admitted while the others run is shown by test_gpu_queue_open.py on the loop's own
clock; a CLI test of it would depend on wall time."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from q3t_testutil import REPO, synth_dir

sys.path.insert(0, os.path.join(REPO, "qwen3-tts-jetson_amd"))
pytestmark = pytest.mark.gpu
CLI = os.path.join(REPO, "qwen3-tts-jetson_amd", "cpp", "qwen3-tts-cli")
MT, SEED, SLOTS = 128, 7, 2
TEXTS = ("This is the first and by far the longest request of the five: it goes on and on, well past the others, "
         "so that it is still running when its neighbours have long finished and been replaced.",
         "Hi.", "This is a test.", "hello world, hello queue", "One more, a little longer than the second one.")
BAD_AFTER = 2   # the malformed request is the third line


def _wav(pcm):   # save_audio_file: PCM16 mono 24 kHz, clamped, scaled by 32767 and truncated toward zero
    data = (np.clip(pcm, -1, 1) * np.float32(32767.0)).astype(np.float32).astype(np.int16).tobytes()
    return (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 24000, 48000, 2, 16)
            + b"data" + struct.pack("<I", len(data)) + data)


@pytest.fixture(scope="module")
def expected():
    """the WAV bytes of every good request from generate_queue + vocoder, computed once"""
    import q3t
    tts, tok = synth_dir("full")
    t = q3t.Tokenizer(tts)
    prompts = [t.encode_for_tts(x) for x in TEXTS]
    t.close()
    eng = q3t.Engine(tts, tok, device=0, max_slots=SLOTS, max_ctx=MT + 40)
    try:
        spk = [np.zeros(eng.cfg["hidden"], np.float32)] * len(TEXTS)
        codes = eng.generate_queue(prompts, speakers=spk, per_utt=[None] * len(TEXTS), max_len=MT, temperature=0.9, top_k=50,
                                   repetition_penalty=1.05, seed=SEED)
        lens = [len(c) for c in codes]
        wavs = [_wav(eng.vocoder(c, 0)) for c in codes]
    finally:
        eng.close()
    return lens, wavs


@pytest.mark.parametrize("extra", [[], ["--stream-full", "4"]], ids=["whole", "stream-full"])
def test_cli_serve_queue_open(tmp_path, expected, extra):
    assert os.path.exists(CLI), "qwen3-tts-cli missing: run __graft_entry__.build()"
    lens, wavs = expected
    assert len(set(lens)) > 1, lens
    tts, tok = synth_dir("full")
    d = tmp_path / "models"   # no chunked engine file: the whole-utterance vocoder
    d.mkdir()
    os.symlink(tts, d / "qwen3-tts-0.6b-f16.gguf")
    os.symlink(tok, d / "qwen3-tts-tokenizer-f16.gguf")
    outs = [str(tmp_path / f"q_{i}.wav") for i in range(len(TEXTS))]
    bad_out = str(tmp_path / "bad.wav")
    lines = [f"{t}\t{o}\n" for t, o in zip(TEXTS, outs)]
    lines.insert(BAD_AFTER, f"never spoken\t{bad_out}\ttemperature=warm\n")
    r = subprocess.run([CLI, "-m", str(d), "--serve", "--queue-open", str(SLOTS), "--max-tokens", str(MT), "--seed", str(SEED)]
                       + extra, input="".join(lines) + "\nquit\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.strip().split("\n")
    ok = [ln for ln in got if ln.split("\t")[0] == "OK"]
    err = [ln for ln in got if ln.split("\t")[0] == "ERR"]
    assert len(ok) == len(TEXTS) and len(err) == 1 and len(got) == len(TEXTS) + 1, r.stdout + r.stderr[-2000:]
    assert "temperature" in err[0] and "warm" in err[0], err
    assert sorted(outs.index(ln.split("\t")[3]) for ln in ok) == list(range(len(TEXTS)))
    assert r.stderr.count("Synthesizing:") == len(TEXTS) and not os.path.exists(bad_out)
    for i, o in enumerate(outs):
        with open(o, "rb") as f:
            wav = f.read()
        assert len(wav) > 44 + 2 * 1000, f"request {i}: (almost) no audio"
        assert wav == wavs[i], f"request {i} ({lens[i]} frames): the WAV differs from generate_queue + vocoder"
