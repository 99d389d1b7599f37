// test_voice_cache.cpp — the voice cache of the serving paths (cpp/voice_cache.h) on the CPU, with a loader and an
// encoder of its own: the misses of one resolve reach the encoder in one call, each file once; a hit does not call it;
// a changed modification time or size is a miss; the capacity evicts the least recently used voice; a failed clip
// reports its message and is not kept.  usage: test_voice_cache <scratch dir>
// Driven by tests/test_voice_cache.py (g++ against the header; no GPU library).
#include <sys/stat.h>
#include <sys/time.h>

#include <cstdio>
#include <string>
#include <vector>

#include "voice_cache.h"

using qwen3_tts::VoiceCache;

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static std::string dir;

// a "clip" file: its bytes are its samples (one float per byte), so the embedding below tells files apart
static std::string put(const std::string &name, const std::string &bytes, long mtime_s) {
    const std::string path = dir + "/" + name;
    FILE *f = fopen(path.c_str(), "wb");
    if (f) { fwrite(bytes.data(), 1, bytes.size(), f); fclose(f); }
    struct timeval tv[2] = {{mtime_s, 0}, {mtime_s, 0}};
    utimes(path.c_str(), tv);
    return path;
}

static int loads = 0, encode_calls = 0;
static std::vector<size_t> encode_sizes;   // clips per encoder call

static bool load(const std::string &path, std::vector<float> &samples, std::string &error) {
    ++loads;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { error = "no such clip " + path; return false; }
    int c;
    samples.clear();
    while ((c = fgetc(f)) != EOF) samples.push_back((float)c);
    fclose(f);
    if (!samples.empty() && samples[0] == (float)'!') { error = "unreadable clip " + path; return false; }
    return true;
}

// embedding = {number of samples, sum of samples}; a clip of fewer than 3 samples is "too short"
static void encode(const std::vector<std::vector<float>> &clips, std::vector<std::vector<float>> &emb,
                   std::vector<std::string> &err) {
    ++encode_calls;
    encode_sizes.push_back(clips.size());
    emb.assign(clips.size(), {});
    err.assign(clips.size(), "");
    for (size_t i = 0; i < clips.size(); ++i) {
        if (clips[i].size() < 3) { err[i] = "clip too short"; continue; }
        float s = 0;
        for (float v : clips[i]) s += v;
        emb[i] = {(float)clips[i].size(), s};
    }
}

static std::vector<float> voice(const std::string &bytes) {
    float s = 0;
    for (unsigned char c : bytes) s += (float)c;
    return {(float)bytes.size(), s};
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: test_voice_cache <scratch dir>\n"); return 2; }
    dir = argv[1];
    const std::string a = put("a.wav", "aaaa", 1000), b = put("b.wav", "bbbbb", 1000), c = put("c.wav", "cccccc", 1000);
    const std::string shorty = put("short.wav", "zz", 1000), broken = put("broken.wav", "!!!!", 1000);
    std::vector<std::vector<float>> emb;
    std::vector<std::string> err;

    {   // ---- the misses of one resolve: one encoder call, each file once, in the order of first mention
        VoiceCache vc(load);
        CHECK(vc.capacity() == 64 && vc.size() == 0);
        vc.resolve({a, b, a, c, b}, encode, emb, err);
        CHECK(encode_calls == 1 && encode_sizes.back() == 3 && loads == 3);
        CHECK(emb.size() == 5 && err.size() == 5);
        for (const std::string &e : err) CHECK(e.empty());
        CHECK(emb[0] == voice("aaaa") && emb[1] == voice("bbbbb") && emb[2] == emb[0] && emb[3] == voice("cccccc") && emb[4] == emb[1]);
        CHECK(vc.size() == 3);
        // ---- hits do not load and do not call the encoder
        vc.resolve({c, a}, encode, emb, err);
        CHECK(encode_calls == 1 && loads == 3 && emb[0] == voice("cccccc") && emb[1] == voice("aaaa") && err[0].empty() && err[1].empty());
        // ---- a mixed set: only the miss is encoded
        const std::string d = put("d.wav", "ddd", 1000);
        vc.resolve({a, d, b}, encode, emb, err);
        CHECK(encode_calls == 2 && encode_sizes.back() == 1 && loads == 4 && emb[1] == voice("ddd") && emb[0] == voice("aaaa"));
        // ---- a changed modification time is a miss (same bytes, same size)
        put("a.wav", "aaaa", 2000);
        vc.resolve({a}, encode, emb, err);
        CHECK(encode_calls == 3 && loads == 5 && emb[0] == voice("aaaa"));
        vc.resolve({a}, encode, emb, err);
        CHECK(encode_calls == 3 && loads == 5);
        // ---- a changed size is a miss (same modification time), and the new content is what comes back
        put("a.wav", "aaaaaaa", 2000);
        vc.resolve({a}, encode, emb, err);
        CHECK(encode_calls == 4 && loads == 6 && emb[0] == voice("aaaaaaa"));
        // ---- an empty set does nothing
        vc.resolve({}, encode, emb, err);
        CHECK(encode_calls == 4 && emb.empty() && err.empty());
    }
    {   // ---- failures: reported per path, not kept, and they do not fail the others
        VoiceCache vc(load);
        const int calls0 = encode_calls, loads0 = loads;
        const std::string missing = dir + "/missing.wav";
        vc.resolve({b, shorty, missing, broken, shorty, c}, encode, emb, err);
        CHECK(encode_calls == calls0 + 1 && encode_sizes.back() == 3);        // b, short, c: the unreadable never reach it
        CHECK(loads == loads0 + 4);                                             // (missing.wav fails at stat)
        CHECK(err[0].empty() && emb[0] == voice("bbbbb") && err[5].empty() && emb[5] == voice("cccccc"));
        CHECK(err[1] == "clip too short" && err[4] == "clip too short" && emb[1].empty() && emb[4].empty());
        CHECK(err[2] == "Failed to load reference audio: " + missing && emb[2].empty());
        CHECK(err[3] == "unreadable clip " + broken && emb[3].empty());
        CHECK(vc.size() == 2);
        // named again: tried again (a miss), while the good ones are hits
        vc.resolve({shorty, b}, encode, emb, err);
        CHECK(encode_calls == calls0 + 2 && encode_sizes.back() == 1 && err[0] == "clip too short" && err[1].empty());
        vc.resolve({broken}, encode, emb, err);
        CHECK(encode_calls == calls0 + 2 && err[0] == "unreadable clip " + broken);   // nothing to encode: no call
    }
    {   // ---- capacity: the least recently used voice leaves
        VoiceCache vc(load, 2);
        CHECK(vc.capacity() == 2);
        vc.resolve({b}, encode, emb, err);
        vc.resolve({c}, encode, emb, err);
        vc.resolve({b}, encode, emb, err);            // b is now the most recently used
        const int calls0 = encode_calls;
        const std::string d = dir + "/d.wav";
        vc.resolve({d}, encode, emb, err);            // evicts c
        CHECK(encode_calls == calls0 + 1 && vc.size() == 2);
        vc.resolve({b}, encode, emb, err);
        CHECK(encode_calls == calls0 + 1);            // still held
        vc.resolve({c}, encode, emb, err);
        CHECK(encode_calls == calls0 + 2 && emb[0] == voice("cccccc"));   // was evicted; comes back and evicts d
        vc.resolve({d}, encode, emb, err);
        CHECK(encode_calls == calls0 + 3 && vc.size() == 2);
        // one resolve with more misses than the capacity: all are answered, the last ones stay
        VoiceCache one(load, 1);
        one.resolve({b, c, d}, encode, emb, err);
        CHECK(emb[0] == voice("bbbbb") && emb[1] == voice("cccccc") && emb[2] == voice("ddd") && one.size() == 1);
        const int calls1 = encode_calls;
        one.resolve({d}, encode, emb, err);
        CHECK(encode_calls == calls1);
    }
    printf(fails ? "%d check(s) failed\n" : "voice_cache: all checks passed\n", fails);
    return fails ? 1 : 0;
}
