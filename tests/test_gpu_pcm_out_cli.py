"""The output stage above the C ABI: qwen3-tts-cli --sample-rate R and the sample_rate=R key of --serve lines
(Qwen3TTS over q3t_vocoder_decode_out / _stream_push_out / _stream_push_batch_out) on the `full` synthetic model, as in
the other CLI tests.  A WAV written with a rate carries it in its header and its data chunk is, byte for byte, the Python
path's (R, S16) output for the same codes; a request without the key next to one with it gets the file it always got;
a bad value fails its own request alone.  The codes come from Engine.generate / generate_queue with the CLI's values
(that they are the CLI's is shown by the 24 kHz files, which must equal the WAV made from them)."""
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
MT, SEED, SLOTS = 40, 5, 2
TEXT = "Hello. This is a test."
TEXTS = ("This is the first request, and the longest of them.", "Hi there.", "never synthesized", "One more, to end with.")
KEYS = ("sample_rate=8000", "", "sample_rate=11025", "top_k=50;sample_rate=48000")     # line 2 is the bad one
GOOD = (0, 1, 3)


def _wav(data, rate):
    return (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16)
            + b"data" + struct.pack("<I", len(data)) + data)


def _wav24(pcm):   # save_audio_file: clamped, scaled by 32767 and truncated toward zero on the host
    return _wav((np.clip(pcm, -1, 1) * np.float32(32767.0)).astype(np.float32).astype(np.int16).tobytes(), 24000)


def _model_dir(tmp_path):
    tts, tok = synth_dir("full")
    d = tmp_path / "models"   # no chunked engine file: the whole-utterance vocoder
    d.mkdir()
    os.symlink(tts, d / "qwen3-tts-0.6b-f16.gguf")
    os.symlink(tok, d / "qwen3-tts-tokenizer-f16.gguf")
    return str(d)


@pytest.fixture(scope="module")
def expected():
    """one-shot: the 24 kHz WAV and the (16000, S16) WAV of TEXT's codes; queue: per good request of TEXTS its 24 kHz
    WAV and the WAVs at 8000 and 48000.  Computed once."""
    import q3t
    tts, tok = synth_dir("full")
    t = q3t.Tokenizer(tts)
    one = t.encode_for_tts(TEXT)
    prompts = [t.encode_for_tts(TEXTS[i]) for i in GOOD]
    t.close()
    eng = q3t.Engine(tts, tok, device=0, max_slots=SLOTS, max_ctx=MT + 40)
    try:
        zero = np.zeros(eng.cfg["hidden"], np.float32)       # the pipeline's zero speaker row
        c = eng.generate([one], speakers=[zero], max_len=MT, temperature=0.9, top_k=50, repetition_penalty=1.05, seed=SEED)[0]
        shot = {24000: _wav24(eng.vocoder(c, 0)), 16000: _wav(eng.vocoder(c, 0, out=(16000, q3t.PCM_S16)).tobytes(), 16000)}
        spk = [np.zeros(eng.cfg["hidden"], np.float32)] * len(GOOD)
        codes = eng.generate_queue(prompts, speakers=spk, max_len=MT, temperature=0.9, top_k=50, repetition_penalty=1.05,
                                   seed=SEED)
        queue = [{24000: _wav24(eng.vocoder(q, 0)),
                  8000: _wav(eng.vocoder(q, 0, out=(8000, q3t.PCM_S16)).tobytes(), 8000),
                  48000: _wav(eng.vocoder(q, 0, out=(48000, q3t.PCM_S16)).tobytes(), 48000)} for q in codes]
    finally:
        eng.close()
    return shot, queue


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_sample_rate_one_shot_and_stream_full(tmp_path, expected):
    assert os.path.exists(CLI), "qwen3-tts-cli missing: run __graft_entry__.build()"
    shot, _ = expected
    d = _model_dir(tmp_path)
    got = {}
    for name, extra in (("plain", []), ("rate", ["--sample-rate", "16000"]),
                        ("rate_stream", ["--sample-rate", "16000", "--stream-full", "7"])):
        out = str(tmp_path / (name + ".wav"))
        r = subprocess.run([CLI, "-m", d, "-t", TEXT, "-o", out, "--max-tokens", str(MT), "--temperature", "0.9",
                            "--seed", str(SEED)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        got[name] = _read(out)
    assert got["plain"] == shot[24000], "without the flag the WAV is what it was (and the codes are Engine.generate's)"
    assert struct.unpack("<I", got["rate"][24:28])[0] == 16000 and struct.unpack("<I", got["rate"][28:32])[0] == 32000
    assert len(got["rate"]) > 44 + 2 * 1000
    assert got["rate"] == shot[16000], "the data chunk is not the Python path's (16000, S16) bytes"
    assert got["rate_stream"] == shot[16000], "--stream-full with a rate: not the one-shot call's bytes"
    # a rate the stage does not have is refused, with its name
    r = subprocess.run([CLI, "-m", d, "-t", TEXT, "-o", str(tmp_path / "bad.wav"), "--max-tokens", "8", "--sample-rate", "11025"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "11025" in r.stderr and not os.path.exists(tmp_path / "bad.wav")


def _serve(tmp_path, d, mode, extra, keys, tag):
    outs = [str(tmp_path / f"{tag}_{i}.wav") for i in range(len(TEXTS))]
    stdin = "".join(f"{t}\t{o}" + (f"\t{k}" if k else "") + "\n" for t, o, k in zip(TEXTS, outs, keys)) + "\nquit\n"
    r = subprocess.run([CLI, "-m", d, "--serve", "--max-tokens", str(MT), "--seed", str(SEED)] + mode + extra,
                       input=stdin, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return outs, [ln for ln in r.stdout.strip().split("\n") if ln], r


@pytest.mark.parametrize("extra", [[], ["--stream-full", "4"]], ids=["whole", "stream-full"])
@pytest.mark.parametrize("mode", [["--queue", str(SLOTS)], ["--queue-open", str(SLOTS)]], ids=["queue", "queue-open"])
def test_cli_serve_sample_rate_key(tmp_path, expected, mode, extra):
    assert os.path.exists(CLI), "qwen3-tts-cli missing: run __graft_entry__.build()"
    _, queue = expected
    d = _model_dir(tmp_path)
    outs, lines, r = _serve(tmp_path, d, mode, extra, KEYS, "k")
    ok = [ln for ln in lines if ln.startswith("OK\t")]
    err = [ln for ln in lines if ln.startswith("ERR\t")]
    assert len(ok) == 3 and len(err) == 1, r.stdout + r.stderr[-2000:]
    assert "11025" in err[0] and "sample_rate" in err[0]               # the bad value failed its own request alone
    assert not os.path.exists(outs[2])
    assert _read(outs[0]) == queue[0][8000], "request 0: not the Python path's (8000, S16) WAV"
    assert struct.unpack("<I", _read(outs[0])[24:28])[0] == 8000
    assert _read(outs[1]) == queue[1][24000], "the request without the key: not the 24 kHz WAV it always got"
    assert _read(outs[3]) == queue[2][48000], "request 3: not the Python path's (48000, S16) WAV"
    # the reported duration is that of the delivered rate
    dur = {ln.split("\t")[3]: float(ln.split("\t")[1]) for ln in ok}
    assert abs(dur[outs[0]] - (len(queue[0][8000]) - 44) / 2 / 8000) < 0.011


@pytest.mark.parametrize("extra", [[], ["--stream-full", "4"]], ids=["whole", "stream-full"])
def test_cli_serve_batch_sample_rate_key(tmp_path, extra):
    """--serve --batch: the lock-step batch has codes of its own, so the reference is the same server without the keys:
    the keyless request's file is identical, and a request with a rate gets that rate's count of the same audio"""
    import q3t
    d = _model_dir(tmp_path)
    mode = ["--batch", "4", "--temperature", "0"]
    outs, lines, r = _serve(tmp_path, d, mode, extra, KEYS, "k")
    base, blines, _ = _serve(tmp_path, d, mode, extra, ("", "", "sample_rate=11025", ""), "b")
    assert sum(ln.startswith("OK\t") for ln in lines) == 3 and sum(ln.startswith("ERR\t") for ln in lines) == 1, r.stdout
    assert sum(ln.startswith("OK\t") for ln in blines) == 3
    assert _read(outs[1]) == _read(base[1])
    for i, rate in ((0, 8000), (3, 48000)):
        got, ref = _read(outs[i]), _read(base[i])
        assert struct.unpack("<II", got[24:32]) == (rate, 2 * rate)
        n24 = (len(ref) - 44) // 2
        assert (len(got) - 44) // 2 == q3t.pcm_num_samples(n24, rate, True) and n24 > 1000
        assert np.abs(np.frombuffer(got[44:], np.int16)).max() > 0
