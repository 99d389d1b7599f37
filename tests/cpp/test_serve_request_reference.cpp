// test_serve_request_reference.cpp — the reference key of a qwen3-tts-cli --serve request line (cpp/serve_request.h)
// on the CPU: it parses next to the other keys, and an empty value, the key given twice, or the key beside speaker=
// fails its request alone, with the text and the output path still set so that the reply can name the request.
// Driven by tests/test_voice_cache.py (g++ against the header; no GPU library).
#include <cstdio>
#include <string>

#include "serve_request.h"

using qwen3_tts::parse_serve_line;
using qwen3_tts::serve_request;

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static bool bad(const std::string &line, const std::string &message) {
    serve_request r;
    std::string err;
    const bool ok = parse_serve_line(line, r, err);
    const bool hit = !ok && err == message && r.text == "hello" && r.output == "o.wav";
    if (!hit) printf("  line '%s': ok=%d error='%s' (wanted '%s')\n", line.c_str(), (int)ok, err.c_str(), message.c_str());
    return hit;
}

int main() {
    serve_request r;
    std::string err;
    // ---- the key parses, alone and among the others
    CHECK(parse_serve_line("hello\to.wav\treference=a.wav", r, err));
    CHECK(err.empty() && r.has_reference && r.reference == "a.wav" && r.any());
    CHECK(!r.has_speaker && r.speaker.empty() && !r.has_language && !r.has_sample_rate && !r.has_max_tokens);
    CHECK(parse_serve_line("hello\to.wav\ttop_k=8;reference=/voices/b c.wav;sample_rate=16000;", r, err));
    CHECK(r.has_reference && r.reference == "/voices/b c.wav" && r.has_top_k && r.top_k == 8 && r.sample_rate == 16000);
    CHECK(parse_serve_line("hello\to.wav\treference=a=b.wav", r, err) && r.reference == "a=b.wav");   // the first '=' splits
    // ---- a line without it is as before
    CHECK(parse_serve_line("hello\to.wav", r, err) && !r.has_reference && r.reference.empty() && !r.any());
    CHECK(parse_serve_line("hello\to.wav\tspeaker=v.embd", r, err) && !r.has_reference && r.has_speaker && r.speaker == "v.embd");
    // ---- an empty value
    CHECK(bad("hello\to.wav\treference=", "bad value '' for request option 'reference'"));
    CHECK(bad("hello\to.wav\ttop_k=3;reference=;language=2050", "bad value '' for request option 'reference'"));
    // ---- given twice
    CHECK(bad("hello\to.wav\treference=a.wav;reference=b.wav", "request option 'reference' given twice"));
    CHECK(bad("hello\to.wav\treference=a.wav;top_k=3;reference=a.wav", "request option 'reference' given twice"));
    // ---- beside speaker=, in either order
    CHECK(bad("hello\to.wav\treference=a.wav;speaker=v.embd", "request options 'speaker' and 'reference' exclude each other"));
    CHECK(bad("hello\to.wav\tspeaker=v.embd;top_k=3;reference=a.wav", "request options 'speaker' and 'reference' exclude each other"));
    // ---- near misses are unknown keys
    CHECK(bad("hello\to.wav\tReference=a.wav", "unknown request option 'Reference'"));
    CHECK(bad("hello\to.wav\treference", "bad request option 'reference' (expected key=value)"));
    printf(fails ? "%d check(s) failed\n" : "serve_request reference: all checks passed\n", fails);
    return fails ? 1 : 0;
}
