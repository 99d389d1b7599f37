// serve_request.h — one request line of qwen3-tts-cli --serve.
//
//   text<TAB>output.wav                      the reference's protocol (src/main.cpp:109-163)
//   text<TAB>output.wav<TAB>key=value;...    the same with values of its own for this request
//
// Keys of the third field: language (a codec language id, or "nothink"), temperature, top_k, repetition_penalty,
// max_tokens, speaker (a raw float32 embedding file, loaded like -e), reference (a WAV clip of the voice, resampled and
// encoded like -r; the server keeps the voices it has met in a small cache; it excludes speaker), sample_rate (the rate of this request's WAV: one
// of 8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000; the device's output stage writes its s16).  A request takes the server's command-line values
// for every key it does not give.  An empty third field gives none.  A bad field (unknown key, missing '=', malformed
// or out-of-range number, a key given twice) fails that request alone with the protocol's ERR reply.
// Header-only and free of the GPU libraries so tests/cpp/test_serve_request.cpp drives it on the CPU.
#ifndef QWEN3_TTS_SERVE_REQUEST_H
#define QWEN3_TTS_SERVE_REQUEST_H

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace qwen3_tts {

struct serve_request {
    std::string text, output;
    // the keys the line gave (has_*) and their values
    bool has_language = false, has_temperature = false, has_top_k = false, has_repetition_penalty = false,
         has_max_tokens = false, has_speaker = false, has_sample_rate = false, has_reference = false;
    int32_t language_id = 2050;   // -1: nothink
    float temperature = 0.0f;
    int32_t top_k = 0;
    float repetition_penalty = 0.0f;
    int32_t max_tokens = 0;
    std::string speaker;          // embedding file
    std::string reference;        // reference clip (WAV)
    int32_t sample_rate = 0;      // Hz, one of the output stage's rates
    bool any() const {
        return has_language || has_temperature || has_top_k || has_repetition_penalty || has_max_tokens || has_speaker ||
               has_sample_rate || has_reference;
    }
};

namespace serve_detail {
inline bool parse_int(const std::string &v, int32_t &out) {
    if (v.empty()) return false;
    errno = 0;
    char *end = nullptr;
    const long x = std::strtol(v.c_str(), &end, 10);
    if (errno != 0 || end != v.c_str() + v.size() || x < INT32_MIN || x > INT32_MAX) return false;
    out = (int32_t)x;
    return true;
}
inline bool parse_float(const std::string &v, float &out) {
    if (v.empty()) return false;
    errno = 0;
    char *end = nullptr;
    const float x = std::strtof(v.c_str(), &end);
    if (errno != 0 || end != v.c_str() + v.size() || !std::isfinite(x)) return false;
    out = x;
    return true;
}
// the rates of the output stage (include/q3t_backend.h)
inline bool known_sample_rate(int32_t r) {
    for (int32_t k : {8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000})
        if (r == k) return true;
    return false;
}
}  // namespace serve_detail

// One line without its line end.  false: the third field is bad, error says why (text and output are set all the
// same, so the caller can name the request in its reply).  A line without a TAB is a text for "output.wav".
inline bool parse_serve_line(const std::string &line, serve_request &r, std::string &error) {
    r = serve_request();
    error.clear();
    const size_t t1 = line.find('\t');
    if (t1 == std::string::npos) { r.text = line; r.output = "output.wav"; return true; }
    r.text = line.substr(0, t1);
    const size_t t2 = line.find('\t', t1 + 1);
    r.output = line.substr(t1 + 1, t2 == std::string::npos ? std::string::npos : t2 - t1 - 1);
    if (t2 == std::string::npos) return true;
    const std::string opts = line.substr(t2 + 1);
    size_t pos = 0;
    while (pos < opts.size()) {
        size_t end = opts.find(';', pos);
        if (end == std::string::npos) end = opts.size();
        const std::string kv = opts.substr(pos, end - pos);
        pos = end + 1;
        if (kv.empty()) continue;   // "a=1;;b=2", a trailing ';'
        const size_t eq = kv.find('=');
        if (eq == std::string::npos || eq == 0) { error = "bad request option '" + kv + "' (expected key=value)"; return false; }
        const std::string key = kv.substr(0, eq), val = kv.substr(eq + 1);
        bool *has = nullptr;
        bool ok = true;
        if (key == "language") {
            has = &r.has_language;
            if (val == "nothink") r.language_id = -1;
            else ok = serve_detail::parse_int(val, r.language_id) && r.language_id >= 0;
        } else if (key == "temperature") {
            has = &r.has_temperature;
            ok = serve_detail::parse_float(val, r.temperature);
        } else if (key == "top_k") {
            has = &r.has_top_k;
            ok = serve_detail::parse_int(val, r.top_k) && r.top_k >= 0;
        } else if (key == "repetition_penalty") {
            has = &r.has_repetition_penalty;
            ok = serve_detail::parse_float(val, r.repetition_penalty) && r.repetition_penalty > 0.0f;
        } else if (key == "max_tokens") {
            has = &r.has_max_tokens;
            ok = serve_detail::parse_int(val, r.max_tokens) && r.max_tokens > 0;
        } else if (key == "speaker") {
            has = &r.has_speaker;
            r.speaker = val;
            ok = !val.empty();
        } else if (key == "reference") {
            has = &r.has_reference;
            ok = !val.empty();
            if (ok && !r.has_reference) r.reference = val;
        } else if (key == "sample_rate") {
            has = &r.has_sample_rate;
            ok = serve_detail::parse_int(val, r.sample_rate) && serve_detail::known_sample_rate(r.sample_rate);
        } else {
            error = "unknown request option '" + key + "'";
            return false;
        }
        if (!ok) { error = "bad value '" + val + "' for request option '" + key + "'"; return false; }
        if (*has) { error = "request option '" + key + "' given twice"; return false; }
        *has = true;
        if (r.has_speaker && r.has_reference) { error = "request options 'speaker' and 'reference' exclude each other"; return false; }
    }
    return true;
}

}  // namespace qwen3_tts

#endif
