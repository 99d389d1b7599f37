"""Incremental text input, the host side (no GPU): the feeder that turns text arriving in pieces into the token ids
of the whole text, the C ABI of q3t_generate_queue_text, and the delivery planner for utterances whose slots may gain
no frame between two ticks.

  feeder    200 random cuts of each of five strings (several spaces in a row, leading and trailing space, a newline,
            non-ASCII bytes cut inside a character): the ids of the pieces concatenate to encode(whole)
  header    q3t_generate_queue_text / q3t_text_cb declared, the symbol exported, the two parameter structs unchanged
  planner   tests/cpp/test_queue_plan_text.cpp against csrc/queue_deliver.h
"""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

from q3t_testutil import REPO, synth_dir

PKG = os.path.join(REPO, "qwen3-tts-jetson_amd")
sys.path.insert(0, PKG)

STRINGS = [
    "Hello world, this is a test.",
    "  two  spaces   and three,  leading and trailing  ",
    "a line\nbreak in the middle\n and after a space",
    "héllo wörld 日本語 naïve 🙂 speech",
    " x",
]


@pytest.fixture(scope="module")
def tok():
    import q3t
    tts, _ = synth_dir("full")
    t = q3t.Tokenizer(tts)
    yield t
    t.close()


def test_feeder_any_cut_gives_the_ids_of_the_whole_text(tok):
    import q3t
    rng = random.Random(5)
    for s in STRINGS:
        raw = s.encode("utf-8")
        whole = tok.encode(raw)
        assert whole, s
        for _ in range(200):
            n_cuts = rng.randint(0, min(8, len(raw)))
            cuts = sorted(rng.randint(0, len(raw)) for _ in range(n_cuts))
            pieces = [raw[a:b] for a, b in zip([0] + cuts, cuts + [len(raw)])]
            fd = q3t.TextFeeder(tok)
            ids = []
            for p in pieces:
                ids += fd.feed(p)
            ids += fd.close()
            assert ids == whole, (s, cuts)
            assert fd.close() == []
    # str pieces as well
    fd = q3t.TextFeeder(tok)
    assert fd.feed("Hello wor") + fd.feed("ld, this is a") + fd.feed(" test.") + fd.close() == tok.encode(STRINGS[0])


def test_feeder_holds_back_the_word_after_the_last_space(tok):
    import q3t
    fd = q3t.TextFeeder(tok)
    assert fd.feed("Hello") == []              # may still grow
    assert fd.feed(" wor") == tok.encode("Hello")
    assert fd.feed("ld") == []
    assert fd.close() == tok.encode(" world")


def test_header_declares_the_text_entry_point():
    import q3t
    hdr = open(os.path.join(REPO, "include", "q3t_backend.h")).read()
    assert re.search(r"typedef\s+int\s+\(\*q3t_text_cb\)\(void \*user, int32_t utt, int32_t frames, int32_t rows_ahead,\s*"
                     r"const int32_t \*\*ids, int32_t \*n_ids, int32_t \*end\);", hdr)
    m = re.search(r"int q3t_generate_queue_text\((.*?)\);", hdr, re.S)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [a.strip().split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["ctx", "n_utt", "tokens", "n_tokens", "speaker", "p", "up", "open", "codes", "n_frames", "held",
                     "max_active", "cb", "user", "interval", "text_cb", "text_user"]
    assert "q3t_generate_queue_text" in q3t.EXPORTS
    lib = C.CDLL(q3t.LIB_PATH)
    assert hasattr(lib, "q3t_generate_queue_text") and hasattr(lib, "q3t_text_feed_stats")
    assert C.sizeof(q3t.GenParams) == 40 and C.sizeof(q3t.UttParams) == 24
    assert callable(q3t.Engine.generate_queue_text)


def test_queue_plan_for_fed_utterances(tmp_path):
    exe = str(tmp_path / "test_queue_plan_text")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tests", "cpp", "test_queue_plan_text.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
