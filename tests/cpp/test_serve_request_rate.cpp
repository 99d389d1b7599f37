// test_serve_request_rate.cpp — the sample_rate key of a qwen3-tts-cli --serve request line (cpp/serve_request.h) on
// the CPU: it parses next to the other keys, and a value that is out of range, malformed or given twice fails its
// request alone, with the text and the output path still set so that the reply can name the request.
// Driven by tests/test_serve_request_rate.py (g++ against the header; no GPU library).
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

static bool bad(const std::string &line, const std::string &needle) {
    serve_request r;
    std::string err;
    const bool ok = parse_serve_line(line, r, err);
    const bool hit = !ok && err.find(needle) != std::string::npos && r.text == "hello" && r.output == "o.wav";
    if (!hit) printf("  line '%s': ok=%d error='%s' (wanted '%s')\n", line.c_str(), (int)ok, err.c_str(), needle.c_str());
    return hit;
}

int main() {
    serve_request r;
    std::string err;
    // ---- the key parses, alone and among the others, for every supported rate
    for (int rate : {8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000}) {
        CHECK(parse_serve_line("hello\to.wav\tsample_rate=" + std::to_string(rate), r, err));
        CHECK(err.empty() && r.has_sample_rate && r.sample_rate == rate && r.any());
        CHECK(!r.has_language && !r.has_temperature && !r.has_top_k && !r.has_max_tokens && !r.has_speaker);
    }
    CHECK(parse_serve_line("hello\to.wav\ttop_k=8;sample_rate=16000;temperature=0.5;", r, err));
    CHECK(r.has_sample_rate && r.sample_rate == 16000 && r.has_top_k && r.top_k == 8 && r.has_temperature);
    // ---- a line without it is as before
    CHECK(parse_serve_line("hello\to.wav", r, err) && !r.has_sample_rate && r.sample_rate == 0 && !r.any());
    CHECK(parse_serve_line("hello\to.wav\ttop_k=8", r, err) && !r.has_sample_rate && r.any());
    // ---- out of range: not one of the output stage's rates
    CHECK(bad("hello\to.wav\tsample_rate=11025", "bad value '11025' for request option 'sample_rate'"));
    CHECK(bad("hello\to.wav\tsample_rate=0", "bad value"));
    CHECK(bad("hello\to.wav\tsample_rate=-8000", "bad value"));
    CHECK(bad("hello\to.wav\tsample_rate=96000", "bad value"));
    CHECK(bad("hello\to.wav\tsample_rate=99999999999999", "bad value"));
    // ---- malformed
    CHECK(bad("hello\to.wav\tsample_rate=", "bad value ''"));
    CHECK(bad("hello\to.wav\tsample_rate=16k", "bad value '16k'"));
    CHECK(bad("hello\to.wav\tsample_rate=16000.0", "bad value"));
    CHECK(bad("hello\to.wav\tsample_rate=16000 ", "bad value"));   // (a leading blank is skipped, as for every integer key)
    CHECK(bad("hello\to.wav\tsample_rate", "expected key=value"));
    CHECK(bad("hello\to.wav\tsample-rate=16000", "unknown request option 'sample-rate'"));
    // ---- given twice
    CHECK(bad("hello\to.wav\tsample_rate=8000;sample_rate=8000", "request option 'sample_rate' given twice"));
    CHECK(bad("hello\to.wav\tsample_rate=8000;top_k=3;sample_rate=16000", "given twice"));
    printf(fails ? "%d check(s) failed\n" : "serve_request sample_rate: all checks passed\n", fails);
    return fails ? 1 : 0;
}
