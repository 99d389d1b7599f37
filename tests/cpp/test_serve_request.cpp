// test_serve_request.cpp — the request-line parser of qwen3-tts-cli --serve (cpp/serve_request.h) on the CPU:
// two-field lines as the reference's protocol reads them, every key of the third field, and the bad fields that must
// fail their request alone.  Driven by tests/test_serve_request.py (g++ against the header; no GPU library).
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
    // ---- two-field lines, and a bare text: as before
    CHECK(parse_serve_line("hello world\tout/a.wav", r, err) && r.text == "hello world" && r.output == "out/a.wav" && !r.any());
    CHECK(err.empty());
    CHECK(parse_serve_line("just text", r, err) && r.text == "just text" && r.output == "output.wav" && !r.any());
    CHECK(parse_serve_line("\tx.wav", r, err) && r.text.empty() && r.output == "x.wav");
    // ---- an empty third field gives nothing
    CHECK(parse_serve_line("hello\to.wav\t", r, err) && r.text == "hello" && r.output == "o.wav" && !r.any());
    CHECK(parse_serve_line("hello\to.wav\t;;", r, err) && !r.any());
    // ---- every key
    CHECK(parse_serve_line("hello\to.wav\tlanguage=2055;temperature=1.3;top_k=8;repetition_penalty=1.2;max_tokens=300;speaker=v/a b.embd",
                           r, err));
    CHECK(r.text == "hello" && r.output == "o.wav" && r.any());
    CHECK(r.has_language && r.language_id == 2055);
    CHECK(r.has_temperature && r.temperature == 1.3f);
    CHECK(r.has_top_k && r.top_k == 8);
    CHECK(r.has_repetition_penalty && r.repetition_penalty == 1.2f);
    CHECK(r.has_max_tokens && r.max_tokens == 300);
    CHECK(r.has_speaker && r.speaker == "v/a b.embd");
    // one key leaves the others unset; temperature 0 (greedy) and top_k 0 (off) are values, not absences
    CHECK(parse_serve_line("hello\to.wav\ttemperature=0", r, err) && r.has_temperature && r.temperature == 0.0f &&
          !r.has_top_k && !r.has_language && !r.has_speaker && !r.has_max_tokens && !r.has_repetition_penalty);
    CHECK(parse_serve_line("hello\to.wav\ttop_k=0;", r, err) && r.has_top_k && r.top_k == 0 && !r.has_temperature);
    CHECK(parse_serve_line("hello\to.wav\tlanguage=nothink", r, err) && r.has_language && r.language_id == -1);
    // a state left by an earlier line does not leak into the next
    CHECK(parse_serve_line("hello\to.wav", r, err) && !r.any() && r.language_id == 2050);
    // ---- bad fields: the request fails alone, text and output still known
    CHECK(bad("hello\to.wav\tvoice=x", "unknown request option 'voice'"));
    CHECK(bad("hello\to.wav\ttemperature=0.9;seed=3", "unknown request option 'seed'"));
    CHECK(bad("hello\to.wav\ttemperature=warm", "bad value 'warm' for request option 'temperature'"));
    CHECK(bad("hello\to.wav\ttemperature=0.9x", "bad value"));
    CHECK(bad("hello\to.wav\ttemperature=", "bad value"));
    CHECK(bad("hello\to.wav\ttemperature=nan", "bad value"));
    CHECK(bad("hello\to.wav\ttop_k=1.5", "bad value '1.5' for request option 'top_k'"));
    CHECK(bad("hello\to.wav\ttop_k=-2", "bad value"));
    CHECK(bad("hello\to.wav\ttop_k=99999999999", "bad value"));
    CHECK(bad("hello\to.wav\trepetition_penalty=0", "bad value"));
    CHECK(bad("hello\to.wav\tmax_tokens=0", "bad value"));
    CHECK(bad("hello\to.wav\tlanguage=english", "bad value 'english'"));
    CHECK(bad("hello\to.wav\tlanguage=-3", "bad value"));
    CHECK(bad("hello\to.wav\tspeaker=", "bad value"));
    CHECK(bad("hello\to.wav\ttemperature", "expected key=value"));
    CHECK(bad("hello\to.wav\t=3", "expected key=value"));
    CHECK(bad("hello\to.wav\ttop_k=4;top_k=5", "given twice"));
    printf(fails ? "%d checks failed\n" : "serve_request: all checks passed\n", fails);
    return fails ? 1 : 0;
}
