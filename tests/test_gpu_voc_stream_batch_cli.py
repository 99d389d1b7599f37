"""The layers above the batched stream push: qwen3-tts-cli --serve --batch 3 --stream-full 7 (Qwen3TTS::synthesize_batch
generating through the frame callback, one vocoder stream per request, every interval's deliveries pushed as one
q3t_vocoder_stream_push_batch) writes the WAVs of the same run without --stream-full, byte for byte."""
import os
import subprocess

import pytest

from q3t_testutil import REPO, synth_dir

pytestmark = pytest.mark.gpu
CLI = os.path.join(REPO, "qwen3-tts-jetson_amd", "cpp", "qwen3-tts-cli")
FR = 24   # tests/test_pipeline.py FR: frames per test utterance (--max-tokens)
TEXTS = ("Hello.", "This is a test.", "hello world")   # the requests of tests/test_pipeline.py::test_cli_serve


def test_cli_serve_batch_stream_full_writes_the_same_wavs(tmp_path):
    assert os.path.exists(CLI), "qwen3-tts-cli missing: run __graft_entry__.build()"
    tts, tok = synth_dir("full")
    d = tmp_path / "models"   # no chunked engine file: the whole-utterance vocoder
    d.mkdir()
    os.symlink(tts, d / "qwen3-tts-0.6b-f16.gguf")
    os.symlink(tok, d / "qwen3-tts-tokenizer-f16.gguf")
    wavs = {}
    for tag, extra in (("plain", []), ("stream", ["--stream-full", "7"])):
        reqs = [(t, str(tmp_path / f"{tag}_{i}.wav")) for i, t in enumerate(TEXTS)]
        stdin = "".join(f"{t}\t{o}\n" for t, o in reqs) + "\nquit\n"
        r = subprocess.run([CLI, "-m", str(d), "--serve", "--batch", "3", "--max-tokens", str(FR), "--temperature", "0"]
                           + extra, input=stdin, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == 3 and all(ln.split("\t")[0] == "OK" for ln in lines), r.stdout + r.stderr[-2000:]
        # the three requests ran as ONE batch (synthesize_batch): all announced before the first is done
        assert r.stderr.count("Synthesizing:") == 3
        assert r.stderr.rindex("Synthesizing:") < r.stderr.index("Done:"), r.stderr[-2000:]
        wavs[tag] = []
        for _, o in reqs:
            with open(o, "rb") as f:
                wavs[tag].append(f.read())
    for i, (a, b) in enumerate(zip(wavs["plain"], wavs["stream"])):
        assert len(a) > 44 + 2 * 1000, f"request {i}: the plain run wrote (almost) no audio"
        assert a == b, f"request {i}: --stream-full changed the WAV"
