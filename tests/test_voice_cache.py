"""The voice cache of the serving paths (qwen3-tts-jetson_amd/cpp/voice_cache.h) and the reference= key of a
qwen3-tts-cli --serve request line (cpp/serve_request.h).  CPU only: tests/cpp/test_voice_cache.cpp and
tests/cpp/test_serve_request_reference.cpp built with g++ against the headers."""
import os
import subprocess

from q3t_testutil import REPO


def _build_and_run(tmp_path, name, *args):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "qwen3-tts-jetson_amd", "cpp"),
                    os.path.join(REPO, "tests", "cpp", name + ".cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


def test_voice_cache(tmp_path):
    clips = tmp_path / "clips"
    clips.mkdir()
    _build_and_run(tmp_path, "test_voice_cache", str(clips))


def test_serve_request_reference_key(tmp_path):
    _build_and_run(tmp_path, "test_serve_request_reference")
