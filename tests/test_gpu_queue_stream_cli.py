"""The layers above the queue deliveries: qwen3-tts-cli --serve --queue 2 (Qwen3TTS::synthesize_queue over
q3t_generate_queue_stream) on the `full` synthetic model (the one whose text vocabulary holds the tokenizer's ids, as in
the other CLI tests; the tiny model's does not), five requests of different lengths through two slots, with and
without --stream-full 4.  Every WAV is byte-identical to the one made from Engine.generate_queue's codes of the same
requests (same seed, two slots) through Engine.vocoder(); there is one OK line per request, each with its output path;
and the reply of a short request comes before that of a longer one that was read earlier."""
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


def _wav(pcm):   # save_audio_file: PCM16 mono 24 kHz, clamped, scaled by 32767 and truncated toward zero
    data = (np.clip(pcm, -1, 1) * np.float32(32767.0)).astype(np.float32).astype(np.int16).tobytes()
    return (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 24000, 48000, 2, 16)
            + b"data" + struct.pack("<I", len(data)) + data)


@pytest.fixture(scope="module")
def expected():
    """the WAV bytes of every request from generate_queue + vocoder, computed once"""
    import q3t
    tts, tok = synth_dir("full")
    t = q3t.Tokenizer(tts)
    prompts = [t.encode_for_tts(x) for x in TEXTS]
    t.close()
    eng = q3t.Engine(tts, tok, device=0, max_slots=SLOTS, max_ctx=MT + 40)
    try:
        spk = [np.zeros(eng.cfg["hidden"], np.float32)] * len(TEXTS)
        codes = eng.generate_queue(prompts, speakers=spk, max_len=MT, temperature=0.9, top_k=50,
                                   repetition_penalty=1.05, seed=SEED)
        lens = [len(c) for c in codes]
        wavs = [_wav(eng.vocoder(c, 0)) for c in codes]
    finally:
        eng.close()
    return lens, wavs


@pytest.mark.parametrize("extra", [[], ["--stream-full", "4"]], ids=["whole", "stream-full"])
def test_cli_serve_queue(tmp_path, expected, extra):
    assert os.path.exists(CLI), "qwen3-tts-cli missing: run __graft_entry__.build()"
    lens, wavs = expected
    assert len(set(lens)) > 1 and lens[1] + 24 < lens[0], f"request 1 must end well before request 0: {lens}"
    tts, tok = synth_dir("full")
    d = tmp_path / "models"   # no chunked engine file: the whole-utterance vocoder
    d.mkdir()
    os.symlink(tts, d / "qwen3-tts-0.6b-f16.gguf")
    os.symlink(tok, d / "qwen3-tts-tokenizer-f16.gguf")
    outs = [str(tmp_path / f"q_{i}.wav") for i in range(len(TEXTS))]
    stdin = "".join(f"{t}\t{o}\n" for t, o in zip(TEXTS, outs)) + "\nquit\n"
    r = subprocess.run([CLI, "-m", str(d), "--serve", "--queue", str(SLOTS), "--max-tokens", str(MT), "--seed", str(SEED)]
                       + extra, input=stdin, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(TEXTS) and all(ln.split("\t")[0] == "OK" for ln in lines), r.stdout + r.stderr[-2000:]
    order = [outs.index(ln.split("\t")[3]) for ln in lines]
    assert sorted(order) == list(range(len(TEXTS))), order
    assert r.stderr.count("Synthesizing:") == len(TEXTS)   # all five were read as one queue
    assert order.index(1) < order.index(0), f"replies came in the order {order}, lengths {lens}"
    for i, o in enumerate(outs):
        with open(o, "rb") as f:
            got = f.read()
        assert len(got) > 44 + 2 * 1000, f"request {i}: (almost) no audio"
        assert got == wavs[i], f"request {i} ({lens[i]} frames): the WAV differs from generate_queue + vocoder"
