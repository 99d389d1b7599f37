// test_voc_stream_api.cpp — drives AudioTokenizerDecoder::stream_begin / stream_decode / stream_end (qwen3_tts_hip.h),
// the C++ mirror of the vocoder stream.  Self-checks the host-side semantics (errors before begin and after end, sample
// counts, the streamed samples equal to decode()'s bit for bit, a second stream on the same decoder) and writes the
// streamed samples to <outdir>/voc_stream.bin for tests/test_gpu_voc_stream_cli.py, which compares them with the
// ctypes path.
//
// usage: test_voc_stream_api <tokenizer.gguf> <outdir>   (<outdir>/voc_codes.bin: int32 codes [F][16])
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "qwen3_tts_hip.h"

using namespace qwen3_tts;

static int g_fail = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                             \
            std::fprintf(stderr, "\n");                                    \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static std::vector<int32_t> read_i32(const std::string &path) {
    std::vector<int32_t> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    int32_t x;
    while (std::fread(&x, 4, 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

static bool stream_all(AudioTokenizerDecoder &d, const std::vector<int32_t> &codes, const std::vector<int> &pieces,
                       std::vector<float> &all) {
    all.clear();
    size_t at = 0;
    std::vector<float> pcm;
    for (int n : pieces) {
        if (!d.stream_decode(codes.data() + at * 16, n, pcm)) return false;
        all.insert(all.end(), pcm.begin(), pcm.end());
        at += (size_t)n;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <tokenizer.gguf> <outdir>\n", argv[0]);
        return 2;
    }
    const std::string tok = argv[1], out = argv[2];
    const std::vector<int32_t> codes = read_i32(out + "/voc_codes.bin");
    const int F = (int)(codes.size() / 16);
    if (F < 30 || codes.size() % 16) {
        std::fprintf(stderr, "missing or short %s/voc_codes.bin\n", out.c_str());
        return 2;
    }
    std::vector<float> pcm, full, streamed;
    {
        AudioTokenizerDecoder d;
        CHECK(!d.stream_begin(64), "stream_begin before load");
        CHECK(d.get_error() == "Model not loaded", "error text '%s'", d.get_error().c_str());
        CHECK(!d.stream_decode(codes.data(), 1, pcm), "stream_decode before load");
        d.stream_end();   // a no-op
    }
    AudioTokenizerDecoder d;
    CHECK(d.load_model(tok), "%s", d.get_error().c_str());
    CHECK(d.decode(codes.data(), F, full), "%s", d.get_error().c_str());
    CHECK(!d.stream_decode(codes.data(), 1, pcm) && pcm.empty(), "stream_decode without stream_begin");
    CHECK(d.stream_begin(F), "%s", d.get_error().c_str());
    CHECK(!d.stream_decode(codes.data(), 0, pcm), "zero frames accepted");
    CHECK(!d.stream_decode(codes.data(), F + 1, pcm), "more than max_frames accepted");
    CHECK(d.get_error().find("exceeds max_frames") != std::string::npos, "error text '%s'", d.get_error().c_str());
    // pieces: single frames, then a one-shot decode in between, then the rest
    std::vector<int> pieces = {1, 1, 11, 7};
    pieces.push_back(F - 20);
    {
        size_t at = 0;
        for (size_t i = 0; i < pieces.size(); ++i) {
            CHECK(d.stream_decode(codes.data() + at * 16, pieces[i], pcm), "%s", d.get_error().c_str());
            streamed.insert(streamed.end(), pcm.begin(), pcm.end());
            at += (size_t)pieces[i];
            if (i == 1) {
                std::vector<float> other;
                CHECK(d.decode(codes.data(), 9, other) && !other.empty(), "one-shot decode between pushes");
                CHECK(std::equal(other.begin(), other.end(), full.begin()), "prefix decode differs");
            }
        }
    }
    CHECK(streamed.size() == full.size(), "streamed %zu samples, decode %zu", streamed.size(), full.size());
    CHECK(streamed.size() == full.size() && std::memcmp(streamed.data(), full.data(), full.size() * 4) == 0,
          "streamed samples differ from decode()");
    CHECK(!d.stream_decode(codes.data(), 1, pcm), "push past max_frames accepted");
    // a new stream_begin drops the open stream and starts from frame 0
    CHECK(d.stream_begin(F), "%s", d.get_error().c_str());
    std::vector<float> again;
    CHECK(stream_all(d, codes, {F}, again), "%s", d.get_error().c_str());
    CHECK(again == full, "second stream differs");
    d.stream_end();
    CHECK(!d.stream_decode(codes.data(), 1, pcm), "stream_decode after stream_end");
    d.unload_model();
    FILE *f = std::fopen((out + "/voc_stream.bin").c_str(), "wb");
    CHECK(f && std::fwrite(streamed.data(), 4, streamed.size(), f) == streamed.size(), "write voc_stream.bin");
    if (f) std::fclose(f);
    if (g_fail) {
        std::printf("FAIL (%d checks)\n", g_fail);
        return 1;
    }
    std::printf("PASS\n");
    return 0;
}
