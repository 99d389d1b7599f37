"""reference=<wav> on the serving paths: qwen3-tts-cli --serve --queue-open 4 and --serve --queue 4 on the `full`
synthetic model, as test_gpu_queue_open_cli.py runs the open queue.  Three requests are piped at once: two name
different 16 kHz PCM16 clips through reference=, one names no voice.  Every WAV is byte-identical to the one the same
server writes when the two voices come as speaker=<embedding file>, the embeddings being Engine.encode_speaker's of the
clips resampled to 24 kHz the way the pipeline does (load_audio_file's s16 / 32768, resample_linear).  A fourth request
whose clip is too short for the encoder gets ERR alone and the others complete."""
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
MT, SLOTS, SR_IN = 6, 4, 16000
TEXTS = ("This is a test.", "hello world, hello queue", "One more, a little longer than the second one.")


def voice_like(n, seed):
    """tests/test_speaker.py's speech-like signal, n samples at SR_IN"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR_IN
    f0 = 140 + 30 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / SR_IN
    x = sum(np.sin(k * ph) / k for k in range(1, 12))
    x *= 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t) ** 2
    x += 0.02 * rng.standard_normal(len(t))
    return (0.3 * x / np.abs(x).max()).astype(np.float32)


def write_wav16(path, x):
    data = np.round(x * 32767.0).astype(np.int16)
    raw = data.tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, SR_IN, 2 * SR_IN, 2, 16)
                + b"data" + struct.pack("<I", len(raw)) + raw)
    return data


def resampled(pcm16):
    """load_audio_file + resample_linear (cpp/qwen3_tts_pipeline.cpp): s16 / 32768 in f32, linear interpolation in f64"""
    x = pcm16.astype(np.float32) / np.float32(32768.0)
    ratio = float(SR_IN) / 24000.0
    n = int(float(len(x)) / ratio)
    src = np.arange(n, dtype=np.float64) * ratio
    i0 = src.astype(np.int64)
    frac = src - i0
    i1 = np.minimum(i0 + 1, len(x) - 1)
    y = ((1.0 - frac) * x[i0].astype(np.float64) + frac * x[i1].astype(np.float64)).astype(np.float32)
    y[i0 + 1 >= len(x)] = x[-1]
    return y


@pytest.fixture(scope="module")
def voices(tmp_path_factory):
    """two reference clips, their embedding files, and a clip too short for the encoder"""
    import q3t
    d = tmp_path_factory.mktemp("voices")
    tts, _ = synth_dir("full")
    eng = q3t.Engine.speaker_only(tts)
    try:
        wavs, embds = [], []
        for i, n in enumerate((SR_IN, SR_IN + 4321)):
            w = str(d / f"voice_{i}.wav")
            pcm = write_wav16(w, voice_like(n, seed=20 + i))
            e = str(d / f"voice_{i}.embd")
            eng.encode_speaker(resampled(pcm)).astype(np.float32).tofile(e)
            wavs.append(w)
            embds.append(e)
    finally:
        eng.close()
    short = str(d / "short.wav")
    write_wav16(short, voice_like(100, seed=3))   # 150 samples at 24 kHz: no mel frame
    models = d / "models"   # no chunked engine file: the whole-utterance vocoder
    models.mkdir()
    tts, tok = synth_dir("full")
    os.symlink(tts, models / "qwen3-tts-0.6b-f16.gguf")
    os.symlink(tok, models / "qwen3-tts-tokenizer-f16.gguf")
    return str(models), wavs, embds, short


def serve(models, mode, lines):
    r = subprocess.run([CLI, "-m", models, "--serve", mode, str(SLOTS), "--max-tokens", str(MT), "--temperature", "0"],
                       input="".join(lines) + "quit\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [ln for ln in r.stdout.strip().split("\n") if ln]
    return [ln for ln in got if ln.startswith("OK\t")], [ln for ln in got if ln.startswith("ERR\t")], r


@pytest.mark.parametrize("mode", ["--queue-open", "--queue"])
def test_cli_serve_reference_key(tmp_path, voices, mode):
    assert os.path.exists(CLI), "qwen3-tts-cli missing: run __graft_entry__.build()"
    models, wavs, embds, short = voices
    ref_out = [str(tmp_path / f"ref_{i}.wav") for i in range(3)]
    emb_out = [str(tmp_path / f"emb_{i}.wav") for i in range(3)]
    bad_out = str(tmp_path / "bad.wav")
    lines = [f"{TEXTS[0]}\t{ref_out[0]}\treference={wavs[0]}\n",
             f"never spoken\t{bad_out}\treference={short}\n",
             f"{TEXTS[1]}\t{ref_out[1]}\n",
             f"{TEXTS[2]}\t{ref_out[2]}\treference={wavs[1]}\n"]
    ok, err, r = serve(models, mode, lines)
    assert len(ok) == 3 and len(err) == 1, r.stdout + r.stderr[-2000:]
    assert "too short" in err[0], err
    assert sorted(ln.split("\t")[3] for ln in ok) == sorted(ref_out) and not os.path.exists(bad_out)
    lines = [f"{TEXTS[0]}\t{emb_out[0]}\tspeaker={embds[0]}\n",
             f"{TEXTS[1]}\t{emb_out[1]}\n",
             f"{TEXTS[2]}\t{emb_out[2]}\tspeaker={embds[1]}\n"]
    ok, err, r = serve(models, mode, lines)
    assert len(ok) == 3 and not err, r.stdout + r.stderr[-2000:]
    for i in range(3):
        with open(ref_out[i], "rb") as f:
            a = f.read()
        with open(emb_out[i], "rb") as f:
            b = f.read()
        assert len(a) > 44 + 2 * 1000, f"request {i}: (almost) no audio"
        assert a == b, f"request {i}: reference= and speaker= give different WAVs"
