// qwen3_tts_pipeline.cpp — TextTokenizer, AudioTokenizerEncoder, Qwen3TTS and the WAV helpers of qwen3_tts_hip.h.
//
// Qwen3TTS drives ONE q3t context (talker + code predictor + vocoder + speaker encoder resident in HBM) the way
// src/qwen3_tts.cpp drives its four components: tokenize -> generate (optionally streaming chunked vocoder decodes
// from the frame callback) -> whole-utterance vocoder, with the same timing / RTF / memory report on stderr.
#include <sys/resource.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "q3t_backend.h"
#include "qwen3_tts_pipeline.h"
#include "voice_cache.h"

namespace qwen3_tts {

namespace {

int64_t now_ms() {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

std::string q3t_error() {
    const char *e = q3t_last_error();
    return e && *e ? std::string(e) : std::string("unknown error");
}

// process memory as the reference samples it on Linux: getrusage max RSS for both figures (qwen3_tts.cpp:29-57)
bool rss_bytes(uint64_t &rss) {
    struct rusage u = {};
    if (getrusage(RUSAGE_SELF, &u) != 0) return false;
    rss = (uint64_t)u.ru_maxrss * 1024ULL;
    return true;
}

std::string format_bytes(uint64_t bytes) {   // qwen3_tts.cpp:59-70
    static const char *units[] = {"B", "KB", "MB", "GB", "TB"};
    double v = (double)bytes;
    int u = 0;
    while (v >= 1024.0 && u < 4) { v /= 1024.0; ++u; }
    char b[64];
    snprintf(b, sizeof b, "%.2f %s", v, units[u]);
    return b;
}

void log_memory(const char *label) {
    uint64_t r = 0;
    if (!rss_bytes(r)) { fprintf(stderr, "  [mem] %-24s unavailable\n", label); return; }
    fprintf(stderr, "  [mem] %-24s rss=%s  phys=%s\n", label, format_bytes(r).c_str(), format_bytes(r).c_str());
}

struct MemSampler {
    tts_result &r;
    bool print;
    void operator()(const char *stage) const {
        uint64_t m = 0;
        if (!rss_bytes(m)) return;
        if (r.mem_rss_start_bytes == 0) { r.mem_rss_start_bytes = m; r.mem_phys_start_bytes = m; }
        r.mem_rss_end_bytes = m;
        r.mem_phys_end_bytes = m;
        r.mem_rss_peak_bytes = std::max(r.mem_rss_peak_bytes, m);
        r.mem_phys_peak_bytes = std::max(r.mem_phys_peak_bytes, m);
        if (print) fprintf(stderr, "  [mem] %-24s rss=%s  phys=%s\n", stage, format_bytes(m).c_str(), format_bytes(m).c_str());
    }
};

// Timing / RTF / memory report, format of qwen3_tts.cpp:536-561
void print_report(const tts_result &r) {
    const double audio_sec = r.sample_rate > 0 ? (double)r.num_samples() / (double)r.sample_rate : 0.0;
    const double wall_sec = (double)r.t_total_ms / 1000.0;
    const double rtf = audio_sec > 0.0 ? wall_sec / audio_sec : 0.0;
    const double xrt = wall_sec > 0.0 ? audio_sec / wall_sec : 0.0;
    fprintf(stderr, "\nTiming:\n");
    fprintf(stderr, "  Tokenization:    %lld ms\n", (long long)r.t_tokenize_ms);
    fprintf(stderr, "  Speaker encode:  %lld ms\n", (long long)r.t_encode_ms);
    fprintf(stderr, "  Code generation: %lld ms\n", (long long)r.t_generate_ms);
    fprintf(stderr, "  Vocoder decode:  %lld ms\n", (long long)r.t_decode_ms);
    fprintf(stderr, "  Total:           %lld ms\n", (long long)r.t_total_ms);
    fprintf(stderr, "  Audio duration:  %.2f s\n", audio_sec);
    fprintf(stderr, "  Throughput:      %.2fx realtime (RTF=%.3f)\n", xrt, rtf);
    fprintf(stderr, "\nMemory:\n");
    fprintf(stderr, "  RSS start/end:   %s -> %s\n", format_bytes(r.mem_rss_start_bytes).c_str(),
            format_bytes(r.mem_rss_end_bytes).c_str());
    fprintf(stderr, "  RSS peak:        %s\n", format_bytes(r.mem_rss_peak_bytes).c_str());
    fprintf(stderr, "  Phys start/end:  %s -> %s\n", format_bytes(r.mem_phys_start_bytes).c_str(),
            format_bytes(r.mem_phys_end_bytes).c_str());
    fprintf(stderr, "  Phys peak:       %s\n", format_bytes(r.mem_phys_peak_bytes).c_str());
}

bool file_exists(const std::string &p) {
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return false;
    fclose(f);
    return true;
}

constexpr int32_t kPrefillLen = 10;   // prefill rows with a speaker row (tts_transformer.cpp:1093-1231)
constexpr int32_t kSampleRate = 24000;
constexpr int32_t kQueueTick = 12;   // synthesize_queue without a stream interval: frames per delivery tick

// ---- the output stage (tts_params::output_sample_rate > 0): the utterance's samples come back from the device as
// s16 at the asked rate (tts_result::pcm16), through q3t_vocoder_decode_out or the _out stream pushes; audio stays empty
bool rate_ok(int32_t rate, int32_t vocoder_chunk, std::string &why) {
    if (rate == 0) return true;
    if (q3t_pcm_num_samples(0, rate, 0) < 0) {
        why = "sample rate " + std::to_string(rate) + " is not supported (supported: 8000, 12000, 16000, 22050, 24000, "
              "32000, 44100, 48000)";
        return false;
    }
    if (vocoder_chunk > 0) { why = "a sample rate needs the whole-utterance vocoder (vocoder chunk 0)"; return false; }
    return true;
}

// a fresh or reset stream takes the utterance's rate, or drops the one of the utterance that held it before
bool set_stream_rate(q3t_voc_stream *v, int32_t rate) {
    const q3t_pcm_spec spec = {rate, Q3T_PCM_S16};
    return q3t_vocoder_stream_set_output(v, rate > 0 ? &spec : nullptr) == Q3T_OK;
}

// one stream's share of an output push: n frames (0 with final: the filter's tail alone), its s16 appended to *pcm
struct OutPiece {
    q3t_voc_stream *st = nullptr;
    const int32_t *codes = nullptr;
    int32_t n = 0, final = 0, rate = 0;
    std::vector<int16_t> *pcm = nullptr;   // one piece per vector and call
};

// ONE q3t_vocoder_stream_push_batch_out over the pieces; on an error no stream has moved and no sample is kept
bool push_out_pieces(q3t_ctx *ctx, const std::vector<OutPiece> &pc, std::string &err) {
    const size_t k = pc.size();
    if (k == 0) return true;
    std::vector<q3t_voc_stream *> st(k);
    std::vector<const int32_t *> cp(k);
    std::vector<int32_t> nf(k), fin(k);
    std::vector<void *> out(k);
    std::vector<int64_t> cap(k), got(k, 0);
    std::vector<size_t> at(k);
    for (size_t j = 0; j < k; ++j) {
        const OutPiece &q = pc[j];
        st[j] = q.st; cp[j] = q.codes; nf[j] = q.n; fin[j] = q.final;
        const int64_t in_total = q3t_vocoder_num_samples(ctx, q3t_vocoder_stream_frames(q.st) + q.n, Q3T_VOCODER_FULL);
        const int64_t n = q3t_pcm_num_samples(in_total, q.rate, q.final) - q3t_vocoder_stream_out_samples(q.st);
        if (in_total < 0 || n < 0) { err = "bad sample count of a vocoder stream"; return false; }
        at[j] = q.pcm->size();
        q.pcm->resize(at[j] + (size_t)n + 1);   // (+ 1: a push of no samples still gets a pointer)
        out[j] = q.pcm->data() + at[j];
        cap[j] = n * 2;
    }
    const int rc = q3t_vocoder_stream_push_batch_out(st.data(), (int32_t)k, cp.data(), nf.data(), fin.data(), out.data(),
                                                     cap.data(), got.data());
    for (size_t j = 0; j < k; ++j) pc[j].pcm->resize(at[j] + (size_t)(rc == Q3T_OK ? got[j] : 0));
    if (rc != Q3T_OK) err = q3t_error();
    return rc == Q3T_OK;
}

// an utterance decoded whole: f32 at 24 kHz into r.audio (FULL, or vocoder_chunk-long chunks), or with a rate the
// device's s16 at that rate into r.pcm16
bool decode_utterance(q3t_ctx *ctx, const int32_t *codes, int32_t nf, int32_t vocoder_chunk, int32_t rate, tts_result &r) {
    int64_t got = 0;
    int rc;
    if (rate > 0) {
        const q3t_pcm_spec spec = {rate, Q3T_PCM_S16};
        const int64_t n = q3t_pcm_num_samples(q3t_vocoder_num_samples(ctx, nf, Q3T_VOCODER_FULL), rate, 1);
        r.pcm16.resize((size_t)std::max<int64_t>(n, 0) + 1);
        rc = q3t_vocoder_decode_out(ctx, codes, nf, Q3T_VOCODER_FULL, &spec, r.pcm16.data(), std::max<int64_t>(n, 0) * 2, &got);
        r.pcm16.resize(rc == Q3T_OK ? (size_t)got : 0);
        return rc == Q3T_OK;
    }
    if (vocoder_chunk > 0) {
        r.audio.resize((size_t)nf * 1920);
        rc = q3t_vocoder_decode_chunked(ctx, codes, nf, 16, vocoder_chunk, r.audio.data(), &got);
    } else {
        r.audio.resize((size_t)std::max<int64_t>(q3t_vocoder_num_samples(ctx, nf, Q3T_VOCODER_FULL), 0));
        rc = q3t_vocoder_decode(ctx, codes, nf, Q3T_VOCODER_FULL, r.audio.data(), &got);
    }
    if (rc != Q3T_OK) return false;
    r.audio.resize((size_t)got);
    return true;
}

struct StreamState {
    q3t_ctx *ctx = nullptr;
    int32_t rate = 0;                        // > 0: the stream has an output spec, the pushes fill *pcm16
    std::vector<int16_t> *pcm16 = nullptr;
    q3t_voc_stream *voc = nullptr;   // set: full_stream_cb pushes into it
    int32_t chunk = 0;
    std::vector<float> *audio = nullptr;
    int64_t decode_ms = 0;
    bool error = false;
    std::string error_msg;
};

// generate_stream callback: decode each delivered chunk with the chunked vocoder (qwen3_tts.cpp:437-453)
int stream_cb(void *user, int32_t /*utt*/, const int32_t *codes, int32_t n_frames, int32_t n_cb) {
    auto *s = static_cast<StreamState *>(user);
    const int64_t t0 = now_ms();
    std::vector<float> pcm((size_t)n_frames * 1920);
    int64_t got = 0;
    if (q3t_vocoder_decode_chunked(s->ctx, codes, n_frames, n_cb, s->chunk, pcm.data(), &got) != Q3T_OK) {
        s->error = true;
        s->error_msg = q3t_error();
        return 0;
    }
    s->audio->insert(s->audio->end(), pcm.begin(), pcm.begin() + got);
    s->decode_ms += now_ms() - t0;
    return 1;
}

// generate_stream callback of --stream-full: push each delivery into the vocoder stream and append what it returns
// (the whole-utterance decode's samples, in order)
int full_stream_cb(void *user, int32_t /*utt*/, const int32_t *codes, int32_t n_frames, int32_t /*n_cb*/) {
    auto *s = static_cast<StreamState *>(user);
    if (n_frames <= 0) return 1;
    const int64_t t0 = now_ms();
    if (s->rate > 0) {
        OutPiece q;
        q.st = s->voc; q.codes = codes; q.n = n_frames; q.rate = s->rate; q.pcm = s->pcm16;
        if (!push_out_pieces(s->ctx, {q}, s->error_msg)) { s->error = true; return 0; }
        s->decode_ms += now_ms() - t0;
        return 1;
    }
    const int64_t total = q3t_vocoder_num_samples(s->ctx, q3t_vocoder_stream_frames(s->voc) + n_frames, Q3T_VOCODER_FULL);
    const int64_t cap = total - q3t_vocoder_stream_samples(s->voc);
    const size_t at = s->audio->size();
    s->audio->resize(at + (size_t)std::max<int64_t>(cap, 0));
    int64_t got = 0;
    if (total < 0 || cap < 0 ||
        q3t_vocoder_stream_push(s->voc, codes, n_frames, s->audio->data() + at, cap, &got) != Q3T_OK) {
        s->audio->resize(at);
        s->error = true;
        s->error_msg = q3t_error();
        return 0;
    }
    s->audio->resize(at + (size_t)got);
    s->decode_ms += now_ms() - t0;
    return 1;
}

// --stream-full for a batch: one vocoder stream per utterance.  The engine delivers the slots of one interval in
// increasing utterance order, so the deliveries are collected (the codes copied: the chunk is pinned memory that is
// reused) until the utterance index stops increasing, and pushed as ONE q3t_vocoder_stream_push_batch.
struct BatchStreamState {
    q3t_ctx *ctx = nullptr;
    std::vector<q3t_voc_stream *> voc;       // per utterance
    std::vector<int32_t> rate;               // per utterance: > 0, its stream has an output spec and fills pcm16
    std::vector<tts_result> *out = nullptr;  // per utterance: audio appended in order
    struct Piece { int32_t utt = 0, n = 0; std::vector<int32_t> codes; };
    std::vector<Piece> pending;
    int64_t decode_ms = 0;
    bool error = false;
    std::string error_msg;

    ~BatchStreamState() {
        for (q3t_voc_stream *v : voc) if (v) q3t_vocoder_stream_close(v);
    }
    bool fail(const std::string &m) {
        error = true;
        error_msg = m;
        pending.clear();
        return false;
    }
    // push the collected deliveries; on an error no stream has moved and no audio is kept from this call
    bool flush() {
        if (error) return false;
        if (pending.empty()) return true;
        const int64_t t0 = now_ms();
        // the pieces of utterances with a sample rate go through the output stage, in a call of their own
        std::vector<OutPiece> op;
        std::vector<Piece> plain;
        for (Piece &q : pending) {
            if (rate[q.utt] <= 0) { plain.push_back(std::move(q)); continue; }
            OutPiece o;
            o.st = voc[q.utt]; o.codes = q.codes.data(); o.n = q.n; o.rate = rate[q.utt]; o.pcm = &(*out)[q.utt].pcm16;
            op.push_back(o);
        }
        std::string why;
        if (!push_out_pieces(ctx, op, why)) return fail(why);
        pending.swap(plain);
        if (pending.empty()) { decode_ms += now_ms() - t0; return true; }
        const size_t k = pending.size();
        std::vector<q3t_voc_stream *> st(k);
        std::vector<const int32_t *> cp(k);
        std::vector<int32_t> nf(k);
        std::vector<float *> pp(k);
        std::vector<int64_t> cap(k), got(k, 0);
        std::vector<size_t> at(k);
        for (size_t j = 0; j < k; ++j) {
            const Piece &q = pending[j];
            st[j] = voc[q.utt];
            cp[j] = q.codes.data();
            nf[j] = q.n;
            const int64_t total = q3t_vocoder_num_samples(ctx, q3t_vocoder_stream_frames(st[j]) + q.n, Q3T_VOCODER_FULL);
            cap[j] = total - q3t_vocoder_stream_samples(st[j]);
            if (total < 0 || cap[j] < 0) return fail("bad sample count of a vocoder stream");
            std::vector<float> &a = (*out)[q.utt].audio;
            at[j] = a.size();
            a.resize(at[j] + (size_t)cap[j]);
            pp[j] = a.data() + at[j];   // one piece per utterance and flush: no later resize moves it
        }
        const int rc = q3t_vocoder_stream_push_batch(st.data(), (int32_t)k, cp.data(), nf.data(), pp.data(), cap.data(), got.data());
        for (size_t j = 0; j < k; ++j) (*out)[pending[j].utt].audio.resize(at[j] + (size_t)(rc == Q3T_OK ? got[j] : 0));
        if (rc != Q3T_OK) return fail(q3t_error());
        pending.clear();
        decode_ms += now_ms() - t0;
        return true;
    }
    // after the generation: the filter's tail of every utterance with a sample rate, in one call
    bool finish() {
        if (error) return false;
        const int64_t t0 = now_ms();
        std::vector<OutPiece> op;
        for (size_t u = 0; u < voc.size(); ++u) {
            if (rate[u] <= 0 || q3t_vocoder_stream_frames(voc[u]) <= 0) continue;
            OutPiece o;
            o.st = voc[u]; o.final = 1; o.rate = rate[u]; o.pcm = &(*out)[u].pcm16;
            op.push_back(o);
        }
        std::string why;
        if (!push_out_pieces(ctx, op, why)) return fail(why);
        decode_ms += now_ms() - t0;
        return true;
    }
};

int batch_full_stream_cb(void *user, int32_t utt, const int32_t *codes, int32_t n_frames, int32_t n_cb) {
    auto *s = static_cast<BatchStreamState *>(user);
    if (s->error) return 0;
    if (n_frames <= 0) return 1;
    if (utt < 0 || utt >= (int32_t)s->voc.size() || n_cb != 16) { s->fail("unexpected delivery from the generate"); return 0; }
    if (!s->pending.empty() && utt <= s->pending.back().utt && !s->flush()) return 0;   // a new interval begins
    BatchStreamState::Piece q;
    q.utt = utt;
    q.n = n_frames;
    q.codes.assign(codes, codes + (size_t)n_frames * 16);
    s->pending.push_back(std::move(q));
    return 1;
}

// synthesize_queue: the deliveries of q3t_generate_queue_stream.  With a stream interval every running utterance
// holds one vocoder stream of a pool that never grows past the slots in use (reset, not reopened, when the next
// utterance takes it) and a callback's pieces go through ONE q3t_vocoder_stream_push_batch; without it the codes are
// kept and decoded at the utterance's final delivery.  The result is handed out at that delivery.
struct QueueSynthState {
    q3t_ctx *ctx = nullptr;
    bool stream_full = false;
    int32_t vocoder_chunk = 0, max_len = 0;
    int64_t t0 = 0;
    std::vector<tts_result> *out = nullptr;
    std::vector<char> reported;
    std::vector<int32_t> n_frames;                  // per utterance, as delivered
    std::vector<double> decode_ms;                  // per utterance: its share of the pushes, or its whole decode
    std::vector<std::vector<int32_t>> codes;        // per utterance (no stream interval)
    std::vector<q3t_voc_stream *> pool, free_list;  // every stream opened; those no utterance holds
    std::vector<q3t_voc_stream *> mine;             // per utterance
    std::vector<int32_t> rate;                      // per utterance: tts_params::output_sample_rate
    const std::function<void(int32_t, const tts_result &)> *on_result = nullptr;
    std::string error_msg;

    ~QueueSynthState() {
        for (q3t_voc_stream *v : pool) q3t_vocoder_stream_close(v);
    }
    void report(int32_t u, bool ok, const std::string &msg) {
        tts_result &r = (*out)[u];
        r.success = ok;
        r.error_msg = msg;
        if (!ok) { r.audio.clear(); r.pcm16.clear(); }
        r.sample_rate = u < (int32_t)rate.size() && rate[u] > 0 ? rate[u] : kSampleRate;
        r.t_total_ms = now_ms() - t0;
        r.t_decode_ms = u < (int32_t)decode_ms.size() ? (int64_t)(decode_ms[u] + 0.5) : 0;
        r.t_generate_ms = std::max<int64_t>(r.t_total_ms - r.t_decode_ms, 0);   // includes the wait for a slot
        reported[u] = 1;
        if (on_result && *on_result) (*on_result)(u, r);
    }
    // the pool: one stream per slot, opened before the queue starts (an open allocates the K/V caches and
    // synchronises the device: not something to do between two frames)
    bool open_pool(int32_t slots) {
        for (int32_t i = 0; i < slots; ++i) {
            q3t_voc_stream *v = nullptr;
            if (q3t_vocoder_stream_open(ctx, max_len, &v) != Q3T_OK) return false;
            pool.push_back(v);
            free_list.push_back(v);
        }
        return true;
    }
    bool take_stream(int32_t u) {   // at most `slots` utterances run at a time, so the pool never runs dry
        if (free_list.empty()) { error_msg = "more utterances in flight than vocoder streams in the pool"; return false; }
        mine[u] = free_list.back();
        free_list.pop_back();
        if (q3t_vocoder_stream_reset(mine[u]) == Q3T_OK && set_stream_rate(mine[u], rate[u])) return true;
        error_msg = "Failed to reset the vocoder stream: " + q3t_error();
        return false;
    }
    bool decode_whole(int32_t u) {
        return decode_utterance(ctx, codes[u].data(), n_frames[u], vocoder_chunk, rate[u], (*out)[u]);
    }
    // one callback: false aborts the queue (error_msg set)
    bool deliver(int32_t n, const int32_t *utt, const int32_t *const *cp, const int32_t *nf, const int32_t *fin) {
        const int64_t td = now_ms();
        std::vector<q3t_voc_stream *> st;
        std::vector<const int32_t *> pc;
        std::vector<int32_t> pn, pu;
        std::vector<float *> pp;
        std::vector<int64_t> cap;
        std::vector<size_t> at;
        std::vector<OutPiece> op;   // the pieces of utterances with a sample rate: a call of their own
        std::vector<int32_t> ou;
        for (int32_t i = 0; i < n; ++i) {
            const int32_t u = utt[i];
            if (u < 0 || u >= (int32_t)out->size() || reported[u]) { error_msg = "unexpected delivery from the queue"; return false; }
            if (stream_full && rate[u] > 0 && (nf[i] > 0 || (fin[i] && mine[u]))) {
                // its frames through the output stage; the final delivery also brings the filter's tail (alone when
                // it carries no frame)
                if (!mine[u] && !take_stream(u)) return false;
                n_frames[u] += std::max(nf[i], 0);
                OutPiece o;
                o.st = mine[u]; o.codes = cp[i]; o.n = std::max(nf[i], 0); o.final = fin[i] ? 1 : 0; o.rate = rate[u];
                o.pcm = &(*out)[u].pcm16;
                op.push_back(o);
                ou.push_back(u);
                continue;
            }
            if (nf[i] <= 0) continue;
            n_frames[u] += nf[i];
            if (!stream_full) { codes[u].insert(codes[u].end(), cp[i], cp[i] + (size_t)nf[i] * 16); continue; }
            if (!mine[u] && !take_stream(u)) return false;
            const int64_t total = q3t_vocoder_num_samples(ctx, q3t_vocoder_stream_frames(mine[u]) + nf[i], Q3T_VOCODER_FULL);
            const int64_t c = total - q3t_vocoder_stream_samples(mine[u]);
            if (total < 0 || c < 0) { error_msg = "bad sample count of a vocoder stream"; return false; }
            std::vector<float> &a = (*out)[u].audio;
            at.push_back(a.size());
            a.resize(a.size() + (size_t)c);
            st.push_back(mine[u]); pc.push_back(cp[i]); pn.push_back(nf[i]); pu.push_back(u); cap.push_back(c);
            pp.push_back(a.data() + at.back());   // one piece per utterance and callback: no later resize moves it
        }
        if (!st.empty()) {
            std::vector<int64_t> got(st.size(), 0);
            const int rc = q3t_vocoder_stream_push_batch(st.data(), (int32_t)st.size(), pc.data(), pn.data(), pp.data(),
                                                         cap.data(), got.data());
            for (size_t j = 0; j < st.size(); ++j) (*out)[pu[j]].audio.resize(at[j] + (size_t)(rc == Q3T_OK ? got[j] : 0));
            if (rc != Q3T_OK) { error_msg = "Vocoder stream decode failed: " + q3t_error(); return false; }
        }
        {
            std::string why;
            if (!push_out_pieces(ctx, op, why)) { error_msg = "Vocoder stream decode failed: " + why; return false; }
            for (size_t j = 0; j < op.size(); ++j) { pu.push_back(ou[j]); pn.push_back(op[j].n); }
        }
        // the batched push serves all its pieces at once: its time is split over them by their frames
        const double push_ms = (double)(now_ms() - td);
        int64_t pushed = 0;
        for (int32_t f : pn) pushed += f;
        for (size_t j = 0; j < pu.size(); ++j) if (pushed > 0) decode_ms[pu[j]] += push_ms * pn[j] / (double)pushed;
        for (int32_t i = 0; i < n; ++i) {
            if (!fin[i]) continue;
            const int32_t u = utt[i];
            if (mine[u]) { free_list.push_back(mine[u]); mine[u] = nullptr; }
            if (n_frames[u] == 0) { report(u, false, "No speech codes generated"); continue; }
            if (!stream_full) {
                const int64_t t = now_ms();
                const bool ok = decode_whole(u);
                decode_ms[u] += (double)(now_ms() - t);
                if (!ok) { report(u, false, "Failed to decode speech codes: " + q3t_error()); continue; }
                std::vector<int32_t>().swap(codes[u]);
            }
            report(u, true, "");
        }
        return true;
    }
};

int queue_synth_cb(void *user, int32_t n, const int32_t *utt, const int32_t *const *codes, const int32_t *n_frames,
                   const int32_t *final, int32_t * /*stop*/) {
    return static_cast<QueueSynthState *>(user)->deliver(n, utt, codes, n_frames, final) ? 1 : 0;
}

// serve_queue(): the open queue's two callbacks.  Requests are numbered as the caller hands them over; the ones the
// engine accepts also get its arrival id, under which their deliveries come.  Only the running utterances are kept
// (`live`): the state does not grow with the requests served.  The vocoder handling is QueueSynthState's.
struct OpenQueueState {
    q3t_ctx *ctx = nullptr;
    bool stream_full = false;
    int32_t vocoder_chunk = 0, max_len = 0, hidden = 0;
    q3t_gen_params p{};
    const TextTokenizer *tokenizer = nullptr;
    const std::function<bool(std::vector<tts_request> &, int32_t, bool)> *next_request = nullptr;
    const std::function<void(int32_t, const tts_result &)> *on_result = nullptr;
    // Qwen3TTS::encode_speakers: the reference clips of one answer, in one batched encode
    std::function<bool(const std::vector<std::string> &, std::vector<std::vector<float>> &, std::vector<std::string> &)> encode_speakers;
    struct Live {
        int32_t request = 0;              // the caller's number
        int32_t rate = 0;                 // tts_params::output_sample_rate of the request
        int32_t n_frames = 0;
        double decode_ms = 0;
        int64_t t0 = 0;
        tts_result r;
        std::vector<int32_t> codes;       // (no stream interval)
        q3t_voc_stream *vs = nullptr;
    };
    std::map<int32_t, Live> live;         // by arrival id
    std::vector<q3t_voc_stream *> pool, free_list;
    std::vector<std::vector<int32_t>> toks;   // what the last answer points into: alive until the next ask
    std::vector<std::vector<float>> spk;
    std::vector<float> zero;
    int32_t next_request_no = 0;
    std::string error_msg;

    ~OpenQueueState() {
        for (q3t_voc_stream *v : pool) q3t_vocoder_stream_close(v);
    }
    void report(Live &l, bool ok, const std::string &msg) {
        tts_result &r = l.r;
        r.success = ok;
        r.error_msg = msg;
        if (!ok) { r.audio.clear(); r.pcm16.clear(); }
        r.sample_rate = l.rate > 0 ? l.rate : kSampleRate;
        r.t_total_ms = now_ms() - l.t0;
        r.t_decode_ms = (int64_t)(l.decode_ms + 0.5);
        r.t_generate_ms = std::max<int64_t>(r.t_total_ms - r.t_decode_ms, 0);
        if (on_result && *on_result) (*on_result)(l.request, r);
    }
    void refuse(int32_t request, const std::string &msg) {   // a request that never enters the queue
        Live l;
        l.request = request;
        l.t0 = now_ms();
        report(l, false, msg);
    }
    bool open_pool(int32_t slots) {
        for (int32_t i = 0; i < slots; ++i) {
            q3t_voc_stream *v = nullptr;
            if (q3t_vocoder_stream_open(ctx, max_len, &v) != Q3T_OK) return false;
            pool.push_back(v);
            free_list.push_back(v);
        }
        return true;
    }
    int arrive(int32_t next_id, int32_t room, int32_t idle, q3t_arrival *out, int32_t *n, int32_t *closed) {
        std::vector<tts_request> reqs;
        const bool more = (*next_request)(reqs, room, idle != 0);
        toks.clear();
        spk.clear();
        // the reference clips of the requests about to be handed out (the first `room`; the others are refused below),
        // resolved here, between two frames, in one batched encode.  One that fails is refused: it takes no arrival id
        // and no room
        std::vector<std::string> ref_paths, ref_err;
        std::vector<std::vector<float>> ref_emb;
        std::vector<int32_t> ref_of(reqs.size(), -1);
        for (size_t i = 0; i < reqs.size() && (int32_t)i < room; ++i)
            if (!reqs[i].reference_audio.empty() && reqs[i].speaker_embedding.empty()) {
                ref_of[i] = (int32_t)ref_paths.size();
                ref_paths.push_back(reqs[i].reference_audio);
            }
        if (!ref_paths.empty() && !(encode_speakers && encode_speakers(ref_paths, ref_emb, ref_err))) {
            ref_err.resize(ref_paths.size());   // nothing could run: every clip fails with the reason
            for (std::string &e : ref_err)
                if (e.empty()) e = "Failed to extract speaker embedding";
        }
        int32_t m = 0;
        for (size_t ri = 0; ri < reqs.size(); ++ri) {
            tts_request &r = reqs[ri];
            const int32_t no = next_request_no++;
            if (m >= room || (int32_t)ri >= room) { refuse(no, "more requests than the queue has room for"); continue; }
            if (!r.reference_audio.empty() && !r.speaker_embedding.empty()) {
                refuse(no, "a request gives its voice as a speaker embedding or as reference audio, not both");
                continue;
            }
            if (ref_of[ri] >= 0) {
                const std::string &why = ref_err[ref_of[ri]];
                if (!why.empty()) { refuse(no, why); continue; }
                r.speaker_embedding = ref_emb[ref_of[ri]];
            }
            if (!r.speaker_embedding.empty() && (int32_t)r.speaker_embedding.size() != hidden) {
                refuse(no, "a speaker embedding must be empty or hold one value per hidden channel");
                continue;
            }
            std::string bad_rate;
            if (!rate_ok(r.params.output_sample_rate, vocoder_chunk, bad_rate)) { refuse(no, bad_rate); continue; }
            const int64_t t = now_ms();
            std::vector<int32_t> ids = tokenizer->encode_for_tts(r.text);
            const int64_t t_tok = now_ms() - t;
            if (ids.empty()) { refuse(no, "Failed to tokenize text"); continue; }
            q3t_arrival &a = out[m];
            a.up.language_id = r.language_id;
            a.up.max_len = std::max(r.params.max_audio_tokens, 1);
            a.up.repetition_penalty = r.params.repetition_penalty;
            a.up.temperature = r.params.temperature;
            a.up.top_k = r.params.top_k;
            a.up.force_frames = 0;
            const float *s = r.speaker_embedding.empty() ? zero.data() : r.speaker_embedding.data();
            // what the engine would refuse fails this request alone (an invalid arrival would end the whole call)
            if (q3t_check_utt(ctx, ids.data(), (int32_t)ids.size(), s, &p, &a.up) != Q3T_OK) { refuse(no, q3t_error()); continue; }
            toks.push_back(std::move(ids));
            spk.emplace_back(s, s + hidden);
            a.key = (uint64_t)(next_id + m);
            Live &l = live[next_id + m];
            l.request = no;
            l.rate = r.params.output_sample_rate;
            l.t0 = now_ms();
            l.r.t_tokenize_ms = t_tok;
            ++m;
        }
        for (int32_t i = 0; i < m; ++i) {   // (the vectors have stopped moving)
            out[i].tokens = toks[i].data();
            out[i].n_tokens = (int32_t)toks[i].size();
            out[i].speaker = spk[i].data();
        }
        *n = m;
        *closed = more ? 0 : 1;
        return 1;
    }
    bool decode_whole(Live &l) {
        return decode_utterance(ctx, l.codes.data(), l.n_frames, vocoder_chunk, l.rate, l.r);
    }
    bool take_stream(Live &l) {
        if (free_list.empty()) { error_msg = "more utterances in flight than vocoder streams in the pool"; return false; }
        l.vs = free_list.back();
        free_list.pop_back();
        if (q3t_vocoder_stream_reset(l.vs) == Q3T_OK && set_stream_rate(l.vs, l.rate)) return true;
        error_msg = "Failed to reset the vocoder stream: " + q3t_error();
        return false;
    }
    // one delivery callback (QueueSynthState::deliver over the live table): false aborts the queue (error_msg set)
    bool deliver(int32_t n, const int32_t *utt, const int32_t *const *cp, const int32_t *nf, const int32_t *fin) {
        const int64_t td = now_ms();
        std::vector<q3t_voc_stream *> st;
        std::vector<const int32_t *> pc;
        std::vector<int32_t> pn;
        std::vector<Live *> pl;
        std::vector<float *> pp;
        std::vector<int64_t> cap;
        std::vector<size_t> at;
        std::vector<OutPiece> op;
        std::vector<Live *> ol;
        for (int32_t i = 0; i < n; ++i) {
            auto it = live.find(utt[i]);
            if (it == live.end()) { error_msg = "unexpected delivery from the queue"; return false; }
            Live &l = it->second;
            if (stream_full && l.rate > 0 && (nf[i] > 0 || (fin[i] && l.vs))) {
                // as QueueSynthState::deliver: the output stage's pieces, the tail with the final delivery
                if (!l.vs && !take_stream(l)) return false;
                l.n_frames += std::max(nf[i], 0);
                OutPiece o;
                o.st = l.vs; o.codes = cp[i]; o.n = std::max(nf[i], 0); o.final = fin[i] ? 1 : 0; o.rate = l.rate;
                o.pcm = &l.r.pcm16;
                op.push_back(o);
                ol.push_back(&l);
                continue;
            }
            if (nf[i] <= 0) continue;
            l.n_frames += nf[i];
            if (!stream_full) { l.codes.insert(l.codes.end(), cp[i], cp[i] + (size_t)nf[i] * 16); continue; }
            if (!l.vs && !take_stream(l)) return false;
            const int64_t total = q3t_vocoder_num_samples(ctx, q3t_vocoder_stream_frames(l.vs) + nf[i], Q3T_VOCODER_FULL);
            const int64_t c = total - q3t_vocoder_stream_samples(l.vs);
            if (total < 0 || c < 0) { error_msg = "bad sample count of a vocoder stream"; return false; }
            std::vector<float> &a = l.r.audio;
            at.push_back(a.size());
            a.resize(a.size() + (size_t)c);
            st.push_back(l.vs); pc.push_back(cp[i]); pn.push_back(nf[i]); pl.push_back(&l); cap.push_back(c);
            pp.push_back(a.data() + at.back());
        }
        if (!st.empty()) {
            std::vector<int64_t> got(st.size(), 0);
            const int rc = q3t_vocoder_stream_push_batch(st.data(), (int32_t)st.size(), pc.data(), pn.data(), pp.data(),
                                                         cap.data(), got.data());
            for (size_t j = 0; j < st.size(); ++j) pl[j]->r.audio.resize(at[j] + (size_t)(rc == Q3T_OK ? got[j] : 0));
            if (rc != Q3T_OK) { error_msg = "Vocoder stream decode failed: " + q3t_error(); return false; }
        }
        {
            std::string why;
            if (!push_out_pieces(ctx, op, why)) { error_msg = "Vocoder stream decode failed: " + why; return false; }
            for (size_t j = 0; j < op.size(); ++j) { pl.push_back(ol[j]); pn.push_back(op[j].n); }
        }
        const double push_ms = (double)(now_ms() - td);
        int64_t pushed = 0;
        for (int32_t f : pn) pushed += f;
        for (size_t j = 0; j < pl.size(); ++j) if (pushed > 0) pl[j]->decode_ms += push_ms * pn[j] / (double)pushed;
        for (int32_t i = 0; i < n; ++i) {
            if (!fin[i]) continue;
            auto it = live.find(utt[i]);
            Live &l = it->second;
            if (l.vs) { free_list.push_back(l.vs); l.vs = nullptr; }
            if (l.n_frames == 0) report(l, false, "No speech codes generated");
            else if (stream_full) report(l, true, "");
            else {
                const int64_t t = now_ms();
                const bool ok = decode_whole(l);
                l.decode_ms += (double)(now_ms() - t);
                report(l, ok, ok ? "" : "Failed to decode speech codes: " + q3t_error());
            }
            live.erase(it);
        }
        return true;
    }
};

int open_queue_arrive(void *user, int32_t next_id, int32_t room, int32_t /*running*/, int32_t idle, q3t_arrival *out,
                      int32_t *n, int32_t *closed) {
    return static_cast<OpenQueueState *>(user)->arrive(next_id, room, idle, out, n, closed);
}
int open_queue_cb(void *user, int32_t n, const int32_t *utt, const int32_t *const *codes, const int32_t *n_frames,
                  const int32_t *final, int32_t * /*stop*/) {
    return static_cast<OpenQueueState *>(user)->deliver(n, utt, codes, n_frames, final) ? 1 : 0;
}

}  // namespace

// ===================================================================================================== Qwen3TTS

Qwen3TTS::Qwen3TTS() = default;
Qwen3TTS::~Qwen3TTS() {
    if (ctx_) q3t_ctx_destroy(ctx_);
}

bool Qwen3TTS::set_device(int device) {
    if (ctx_) { error_msg_ = "set_device must precede load_models"; return false; }
    device_ = device;
    return true;
}

bool Qwen3TTS::load_models(const std::string &model_dir) {
    const int64_t t_start = now_ms();
    log_memory("load/start");
    if (ctx_) { q3t_ctx_destroy(ctx_); ctx_ = nullptr; }
    models_loaded_ = false;
    tts_model_path_ = model_dir + "/qwen3-tts-0.6b-f16.gguf";
    decoder_model_path_ = model_dir + "/qwen3-tts-tokenizer-f16.gguf";
    const char *low = std::getenv("QWEN3_TTS_LOW_MEM");
    if (low && low[0] != '\0' && low[0] != '0')
        fprintf(stderr, "  Low-memory mode requested: ignored (all models stay resident in HBM)\n");
    fprintf(stderr, "Loading TTS model from %s...\n", tts_model_path_.c_str());
    const int64_t t_tok = now_ms();
    if (!tokenizer_.load_from_gguf(tts_model_path_)) {
        error_msg_ = "Failed to load text tokenizer: " + tokenizer_.get_error();
        return false;
    }
    fprintf(stderr, "  Text tokenizer loaded: vocab_size=%d (%lld ms)\n", tokenizer_.get_config().vocab_size,
            (long long)(now_ms() - t_tok));
    log_memory("load/after-tokenizer");
    // vocoder choice in the reference's order (qwen3_tts.cpp:168-218): a chunked "TRT" engine file if present
    if (vocoder_chunk_ == 0) {
        if (file_exists(model_dir + "/vocoder_decoder_40.trt")) vocoder_chunk_ = 40;
        else if (file_exists(model_dir + "/vocoder_decoder_30.trt")) vocoder_chunk_ = 30;
        else if (file_exists(model_dir + "/vocoder_decoder_fixed.trt")) vocoder_chunk_ = 20;
    }
    const int64_t t_model = now_ms();
    slots_ = 1;
    n_ctx_ = kPrefillLen + 4096 + 8;
    if (q3t_ctx_create(tts_model_path_.c_str(), decoder_model_path_.c_str(), device_, slots_, n_ctx_, &ctx_) != Q3T_OK) {
        ctx_ = nullptr;
        error_msg_ = "Failed to load TTS transformer: " + q3t_error();
        return false;
    }
    q3t_config c;
    q3t_get_config(ctx_, &c);
    hidden_ = c.hidden;
    codec_vocab_ = c.codec_vocab;
    fprintf(stderr, "  TTS transformer loaded: hidden_size=%d, n_layers=%d (%lld ms)\n", c.hidden, c.n_layers,
            (long long)(now_ms() - t_model));
    if (vocoder_chunk_ > 0)
        fprintf(stderr, "  Chunked vocoder ready: %d fixed frames (%.1f s max per chunk)\n", vocoder_chunk_,
                vocoder_chunk_ / 12.5f);
    else
        fprintf(stderr, "  Vocoder loaded: sample_rate=%d, n_codebooks=%d\n", c.sample_rate, c.n_codebooks);
    if (q3t_speaker_dim(ctx_) > 0) fprintf(stderr, "  Speaker encoder: resident (dim %d)\n", q3t_speaker_dim(ctx_));
    models_loaded_ = true;
    fprintf(stderr, "All models loaded in %lld ms\n", (long long)(now_ms() - t_start));
    log_memory("load/end");
    return true;
}

bool Qwen3TTS::ensure_slots(int32_t slots, int32_t max_len) {
    const int32_t n_ctx = kPrefillLen + max_len + 8;
    if (slots <= slots_ && n_ctx <= n_ctx_) return true;
    q3t_ctx *grown = nullptr;
    const int32_t s = std::max(slots, slots_), n = std::max(n_ctx, n_ctx_);
    if (q3t_ctx_create_replica(ctx_, device_, s, n, &grown) != Q3T_OK) { error_msg_ = q3t_error(); return false; }
    q3t_ctx_destroy(ctx_);
    ctx_ = grown;
    slots_ = s;
    n_ctx_ = n;
    return true;
}

tts_result Qwen3TTS::synthesize(const std::string &text, const tts_params &params) {
    tts_result result;
    if (!models_loaded_) { result.error_msg = "Models not loaded"; return result; }
    // a zero speaker row, not an absent one (qwen3_tts.cpp:241-245)
    std::vector<float> zero(hidden_, 0.0f);
    return synthesize_internal(text, zero.data(), params, result);
}

tts_result Qwen3TTS::synthesize_with_voice(const std::string &text, const std::string &reference_audio,
                                           const tts_params &params) {
    tts_result result;
    std::vector<float> ref;
    int sr = 0;
    if (!load_audio_file(reference_audio, ref, sr)) {
        result.error_msg = "Failed to load reference audio: " + reference_audio;
        return result;
    }
    if (sr != kSampleRate) {
        fprintf(stderr, "Resampling audio from %d Hz to %d Hz...\n", sr, kSampleRate);
        std::vector<float> rs;
        resample_linear(ref.data(), (int)ref.size(), sr, rs, kSampleRate);
        ref.swap(rs);
    }
    return synthesize_with_voice(text, ref.data(), (int32_t)ref.size(), params);
}

tts_result Qwen3TTS::synthesize_with_voice(const std::string &text, const float *ref_samples, int32_t n_ref_samples,
                                           const tts_params &params) {
    tts_result result;
    if (!models_loaded_) { result.error_msg = "Models not loaded"; return result; }
    const int32_t dim = q3t_speaker_dim(ctx_);
    if (dim <= 0) { result.error_msg = "Failed to load speaker encoder: No speaker encoder tensors found in model"; return result; }
    const int64_t t0 = now_ms();
    std::vector<float> emb(dim);
    if (q3t_speaker_encode(ctx_, ref_samples, n_ref_samples, emb.data()) != Q3T_OK) {
        result.error_msg = "Failed to extract speaker embedding: " + q3t_error();
        return result;
    }
    result.t_encode_ms = now_ms() - t0;
    if (params.print_progress) fprintf(stderr, "Speaker embedding extracted: %zu floats\n", emb.size());
    return synthesize_internal(text, emb.data(), params, result);
}

bool Qwen3TTS::encode_speaker(const std::string &reference_audio, std::vector<float> &embedding) {
    if (!models_loaded_) { error_msg_ = "Models not loaded"; return false; }
    std::vector<float> ref;
    int sr = 0;
    if (!load_audio_file(reference_audio, ref, sr)) {
        error_msg_ = "Failed to load reference audio: " + reference_audio;
        return false;
    }
    if (sr != kSampleRate) {
        std::vector<float> rs;
        resample_linear(ref.data(), (int)ref.size(), sr, rs, kSampleRate);
        ref.swap(rs);
    }
    const int32_t dim = q3t_speaker_dim(ctx_);
    if (dim <= 0) { error_msg_ = "Failed to load speaker encoder: No speaker encoder tensors found in model"; return false; }
    embedding.resize(dim);
    if (q3t_speaker_encode(ctx_, ref.data(), (int32_t)ref.size(), embedding.data()) != Q3T_OK) {
        error_msg_ = "Failed to extract speaker embedding: " + q3t_error();
        return false;
    }
    return true;
}

bool Qwen3TTS::encode_speakers(const std::vector<std::string> &reference_audios, std::vector<std::vector<float>> &embeddings,
                               std::vector<std::string> &errors) {
    embeddings.assign(reference_audios.size(), {});
    errors.assign(reference_audios.size(), "");
    if (!models_loaded_) { error_msg_ = "Models not loaded"; errors.assign(errors.size(), error_msg_); return false; }
    const int32_t dim = q3t_speaker_dim(ctx_);
    if (dim <= 0) {
        error_msg_ = "Failed to load speaker encoder: No speaker encoder tensors found in model";
        errors.assign(errors.size(), error_msg_);
        return false;
    }
    if (!voices_)   // the loader is encode_speaker's: the reference's linear resampling to 24 kHz
        voices_.reset(new VoiceCache([](const std::string &path, std::vector<float> &samples, std::string &error) {
            int sr = 0;
            if (!load_audio_file(path, samples, sr)) { error = "Failed to load reference audio: " + path; return false; }
            if (sr != kSampleRate) {
                std::vector<float> rs;
                resample_linear(samples.data(), (int)samples.size(), sr, rs, kSampleRate);
                samples.swap(rs);
            }
            return true;
        }));
    bool ran = true;
    voices_->resolve(reference_audios, [&](const std::vector<std::vector<float>> &clips, std::vector<std::vector<float>> &emb,
                                           std::vector<std::string> &err) {
        const int32_t n = (int32_t)clips.size();
        std::vector<const float *> ptr(n);
        std::vector<int32_t> len(n), ok(n, 0);
        for (int32_t i = 0; i < n; ++i) { ptr[i] = clips[i].data(); len[i] = (int32_t)clips[i].size(); }
        std::vector<float> flat((size_t)n * dim);
        emb.assign(n, {});
        err.assign(n, "");
        if (q3t_speaker_encode_batch(ctx_, ptr.data(), len.data(), n, flat.data(), ok.data()) != Q3T_OK) {
            ran = false;
            error_msg_ = "Failed to extract speaker embedding: " + q3t_error();
            err.assign(n, error_msg_);
            return;
        }
        for (int32_t i = 0; i < n; ++i) {
            if (ok[i]) emb[i].assign(flat.begin() + (size_t)i * dim, flat.begin() + (size_t)(i + 1) * dim);
            else err[i] = "Failed to extract speaker embedding: Audio too short for the speaker encoder";
        }
    }, embeddings, errors);
    return ran;
}

void Qwen3TTS::resolve_references(const std::vector<tts_request> &requests, std::vector<tts_request> &run,
                                  std::vector<int32_t> &index, std::vector<std::string> &failed) {
    failed.assign(requests.size(), "");
    std::vector<std::string> paths, err;
    std::vector<int32_t> at(requests.size(), -1);
    for (size_t i = 0; i < requests.size(); ++i) {
        if (requests[i].reference_audio.empty()) continue;
        if (!requests[i].speaker_embedding.empty()) {
            failed[i] = "a request gives its voice as a speaker embedding or as reference audio, not both";
            continue;
        }
        at[i] = (int32_t)paths.size();
        paths.push_back(requests[i].reference_audio);
    }
    std::vector<std::vector<float>> emb;
    const bool ran = paths.empty() || encode_speakers(paths, emb, err);
    for (size_t i = 0; i < requests.size(); ++i) {
        if (at[i] >= 0) failed[i] = !ran ? error_msg_ : err[at[i]];
        if (!failed[i].empty()) continue;
        run.push_back(requests[i]);
        if (at[i] >= 0) run.back().speaker_embedding = emb[at[i]];
        index.push_back((int32_t)i);
    }
}

tts_result Qwen3TTS::synthesize_with_embedding(const std::string &text, const std::vector<float> &speaker_embedding,
                                               const tts_params &params) {
    tts_result result;
    if (!models_loaded_) { result.error_msg = "Models not loaded"; return result; }
    return synthesize_internal(text, speaker_embedding.data(), params, result);
}

tts_result Qwen3TTS::synthesize_internal(const std::string &text, const float *speaker_embedding,
                                         const tts_params &params, tts_result &result) {
    const int64_t t_total = now_ms();
    MemSampler mem{result, params.print_timing};
    mem("synth/start");
    const int64_t t_tok = now_ms();
    std::vector<int32_t> tokens = tokenizer_.encode_for_tts(text);
    result.t_tokenize_ms = now_ms() - t_tok;
    mem("synth/after-tokenize");
    if (tokens.empty()) { result.error_msg = "Failed to tokenize text"; return result; }
    if (params.print_progress) {
        fprintf(stderr, "Text tokenized: %zu tokens\n", tokens.size());
        fprintf(stderr, "  Tokens: ");
        for (size_t i = 0; i < std::min(tokens.size(), (size_t)10); ++i) fprintf(stderr, "%d ", tokens[i]);
        if (tokens.size() > 10) fprintf(stderr, "...");
        fprintf(stderr, "\n");
    }
    const int32_t rate = params.output_sample_rate;
    if (!rate_ok(rate, vocoder_chunk_, result.error_msg)) return result;
    const int64_t t_gen = now_ms();
    const int32_t max_len = std::max(params.max_audio_tokens, 0);
    if (!ensure_slots(1, std::max(max_len, 1))) { result.error_msg = "Failed to generate speech codes: " + error_msg_; return result; }
    q3t_gen_params p;
    q3t_default_params(&p);
    p.max_len = max_len;
    p.language_id = 2050;
    p.repetition_penalty = params.repetition_penalty;
    p.temperature = params.temperature;
    p.top_k = params.top_k;
    p.seed = seed_;
    std::vector<int32_t> codes((size_t)std::max(max_len, 1) * 16);
    int32_t n_frames = 0, n_tok = (int32_t)tokens.size();
    const int32_t *tok_ptr[1] = {tokens.data()};
    const float *spk[1] = {speaker_embedding};
    StreamState st;
    st.ctx = ctx_;
    st.chunk = vocoder_chunk_;
    st.audio = &result.audio;
    st.rate = rate;
    st.pcm16 = &result.pcm16;
    const bool stream_full = stream_full_ > 0 && vocoder_chunk_ <= 0 && max_len > 0;
    if (stream_full && q3t_vocoder_stream_open(ctx_, max_len, &st.voc) != Q3T_OK) {
        result.error_msg = "Failed to open the vocoder stream: " + q3t_error();
        return result;
    }
    if (st.voc && rate > 0 && !set_stream_rate(st.voc, rate)) {
        result.error_msg = "Failed to open the vocoder stream: " + q3t_error();
        q3t_vocoder_stream_close(st.voc);
        return result;
    }
    int rc;
    if (max_len == 0) rc = Q3T_OK;
    else if (vocoder_chunk_ > 0)
        rc = q3t_generate_stream(ctx_, 1, tok_ptr, &n_tok, speaker_embedding ? spk : nullptr, &p, codes.data(),
                                 &n_frames, stream_cb, &st, 40);
    else if (stream_full)
        rc = q3t_generate_stream(ctx_, 1, tok_ptr, &n_tok, speaker_embedding ? spk : nullptr, &p, codes.data(),
                                 &n_frames, full_stream_cb, &st, stream_full_);
    else
        rc = q3t_generate(ctx_, 1, tok_ptr, &n_tok, speaker_embedding ? spk : nullptr, &p, codes.data(), &n_frames);
    if (st.voc && rc == Q3T_OK && !st.error && q3t_vocoder_stream_frames(st.voc) != n_frames) {
        st.error = true;
        st.error_msg = "the callback saw " + std::to_string(q3t_vocoder_stream_frames(st.voc)) + " of " +
                       std::to_string(n_frames) + " generated frames";
    }
    if (st.voc && rate > 0 && rc == Q3T_OK && !st.error && n_frames > 0) {   // the filter's tail
        OutPiece q;
        q.st = st.voc; q.final = 1; q.rate = rate; q.pcm = &result.pcm16;
        const int64_t t0 = now_ms();
        if (!push_out_pieces(ctx_, {q}, st.error_msg)) st.error = true;
        st.decode_ms += now_ms() - t0;
    }
    if (st.voc) q3t_vocoder_stream_close(st.voc);
    if (rc != Q3T_OK) { result.error_msg = "Failed to generate speech codes: " + q3t_error(); return result; }
    if (st.error) {
        result.error_msg = (stream_full ? "Vocoder stream decode failed: " : "TRT vocoder decode failed: ") + st.error_msg;
        return result;
    }
    result.t_generate_ms = now_ms() - t_gen;
    mem("synth/after-generate");
    if (params.print_progress) fprintf(stderr, "Speech codes generated: %d frames x %d codebooks\n", n_frames, 16);
    if (n_frames == 0) { result.error_msg = "No speech codes generated"; return result; }
    const int64_t t_dec = now_ms();
    if (vocoder_chunk_ <= 0 && !stream_full && rate > 0) {
        if (!decode_utterance(ctx_, codes.data(), n_frames, 0, rate, result)) {
            result.error_msg = "Failed to decode speech codes: " + q3t_error();
            return result;
        }
    } else if (vocoder_chunk_ <= 0 && !stream_full) {
        const int64_t n = q3t_vocoder_num_samples(ctx_, n_frames, Q3T_VOCODER_FULL);
        result.audio.resize((size_t)std::max<int64_t>(n, 0));
        int64_t got = 0;
        if (n < 0 || q3t_vocoder_decode(ctx_, codes.data(), n_frames, Q3T_VOCODER_FULL, result.audio.data(), &got) != Q3T_OK) {
            result.error_msg = "Failed to decode speech codes: " + q3t_error();
            return result;
        }
        result.audio.resize((size_t)got);
    }
    result.sample_rate = rate > 0 ? rate : kSampleRate;
    result.t_decode_ms = st.decode_ms + (now_ms() - t_dec);
    mem("synth/after-decode");
    result.success = true;
    result.t_total_ms = now_ms() - t_total;
    mem("synth/end");
    if (params.print_timing) print_report(result);
    return result;
}

// the requests of the text / embedding overloads: one tts_params for all
static std::vector<tts_request> uniform_requests(const std::vector<std::string> &texts,
                                                 const std::vector<std::vector<float>> &speaker_embeddings,
                                                 const tts_params &params) {
    std::vector<tts_request> reqs(texts.size());
    for (size_t i = 0; i < texts.size(); ++i) {
        reqs[i].text = texts[i];
        reqs[i].params = params;
        if (!speaker_embeddings.empty()) reqs[i].speaker_embedding = speaker_embeddings[i];
    }
    return reqs;
}

// what q3t_generate_utt / q3t_generate_queue_utt would refuse for this request -- and with it every request of the set
bool Qwen3TTS::check_request(const tts_request &r, std::string &error) const {
    error.clear();
    if (!models_loaded_) error = "Models not loaded";
    else if (r.language_id >= codec_vocab_) error = "language id " + std::to_string(r.language_id) + " out of range";
    else if (r.params.top_k < 0) error = "top_k must be >= 0";
    else if (!(r.params.repetition_penalty > 0.0f) || !std::isfinite(r.params.repetition_penalty))
        error = "repetition_penalty must be finite and > 0";
    else if (!std::isfinite(r.params.temperature)) error = "temperature must be finite";
    else if (!r.reference_audio.empty() && !r.speaker_embedding.empty())
        error = "a request gives its voice as a speaker embedding or as reference audio, not both";
    else if (!r.speaker_embedding.empty() && (int32_t)r.speaker_embedding.size() != hidden_)
        error = "speaker embedding holds " + std::to_string(r.speaker_embedding.size()) + " values, the model needs " +
                std::to_string(hidden_);
    else rate_ok(r.params.output_sample_rate, vocoder_chunk_, error);
    return error.empty();
}

// one q3t_utt_params per request, and the call's q3t_gen_params (max_len: the longest request's)
static void request_params(const std::vector<tts_request> &reqs, uint64_t seed, q3t_gen_params &p, std::vector<q3t_utt_params> &up) {
    q3t_default_params(&p);
    p.seed = seed;
    p.max_len = 1;
    up.resize(reqs.size());
    for (size_t i = 0; i < reqs.size(); ++i) {
        const tts_params &tp = reqs[i].params;
        up[i].language_id = reqs[i].language_id;
        up[i].max_len = std::max(tp.max_audio_tokens, 1);
        up[i].repetition_penalty = tp.repetition_penalty;
        up[i].temperature = tp.temperature;
        up[i].top_k = tp.top_k;
        up[i].force_frames = 0;
        p.max_len = std::max(p.max_len, up[i].max_len);
    }
}

std::vector<tts_result> Qwen3TTS::synthesize_batch(const std::vector<std::string> &texts,
                                                   const std::vector<std::vector<float>> &speaker_embeddings,
                                                   const tts_params &params) {
    const bool bad = !speaker_embeddings.empty() && speaker_embeddings.size() != texts.size();
    return batch_requests(uniform_requests(texts, bad ? std::vector<std::vector<float>>() : speaker_embeddings, params),
                          bad ? "speaker_embeddings must be empty or hold one entry per text" : "");
}

static bool any_reference(const std::vector<tts_request> &requests) {
    for (const tts_request &r : requests)
        if (!r.reference_audio.empty()) return true;
    return false;
}

std::vector<tts_result> Qwen3TTS::synthesize_batch(const std::vector<tts_request> &requests) {
    if (!models_loaded_ || !any_reference(requests)) return batch_requests(requests, "");
    // the reference clips of the call in one batched encode; a request whose clip fails ends here, the rest run
    std::vector<tts_request> run;
    std::vector<int32_t> index;
    std::vector<std::string> failed;
    const int64_t t0 = now_ms();
    resolve_references(requests, run, index, failed);
    const int64_t t_enc = now_ms() - t0;
    std::vector<tts_result> out(requests.size());
    for (size_t i = 0; i < requests.size(); ++i) out[i].error_msg = failed[i];
    const std::vector<tts_result> res = batch_requests(run, "");
    for (size_t j = 0; j < res.size(); ++j) { out[index[j]] = res[j]; out[index[j]].t_encode_ms = t_enc; }
    return out;
}

// arg_error: what the caller found wrong with its arguments (reported after the "Models not loaded" check, as before)
std::vector<tts_result> Qwen3TTS::batch_requests(const std::vector<tts_request> &requests, const std::string &arg_error) {
    const int32_t n = (int32_t)requests.size();
    std::vector<tts_result> out(n);
    auto fail_all = [&](const std::string &m) {
        for (auto &r : out) r.error_msg = m;
        return out;
    };
    if (!models_loaded_) return fail_all("Models not loaded");
    if (n == 0) return out;
    if (!arg_error.empty()) return fail_all(arg_error);
    for (const tts_request &r : requests)
        if (!r.speaker_embedding.empty() && (int32_t)r.speaker_embedding.size() != hidden_)
            return fail_all("a speaker embedding must be empty or hold one value per hidden channel");
    std::string bad_rate;
    for (const tts_request &r : requests)
        if (!rate_ok(r.params.output_sample_rate, vocoder_chunk_, bad_rate)) return fail_all(bad_rate);
    const int64_t t0 = now_ms();
    std::vector<std::vector<int32_t>> toks(n);
    std::vector<const int32_t *> tp(n);
    std::vector<int32_t> nt(n), nf(n);
    const std::vector<float> zero(hidden_, 0.0f);   // no embedding: a zero speaker row, as in every call of this pipeline
    std::vector<const float *> spk(n);
    for (int32_t i = 0; i < n; ++i) {
        const int64_t t = now_ms();
        toks[i] = tokenizer_.encode_for_tts(requests[i].text);
        out[i].t_tokenize_ms = now_ms() - t;
        if (toks[i].empty()) return fail_all("Failed to tokenize text");
        tp[i] = toks[i].data();
        nt[i] = (int32_t)toks[i].size();
        spk[i] = requests[i].speaker_embedding.empty() ? zero.data() : requests[i].speaker_embedding.data();
    }
    q3t_gen_params p;
    std::vector<q3t_utt_params> up;
    request_params(requests, seed_, p, up);
    const int32_t max_len = p.max_len;
    if (!ensure_slots(n, max_len)) return fail_all("Failed to generate speech codes: " + error_msg_);
    std::vector<int32_t> codes((size_t)n * max_len * 16);
    // --stream-full: one vocoder stream per utterance, the deliveries of an interval pushed as one batch while the
    // generation runs; the audio is the whole-utterance FULL decode's, sample for sample
    const bool stream_full = stream_full_ > 0 && vocoder_chunk_ <= 0;
    BatchStreamState bs;   // closes its streams on every path
    if (stream_full) {
        bs.ctx = ctx_;
        bs.out = &out;
        bs.voc.assign(n, nullptr);
        bs.rate.assign(n, 0);
        for (int32_t i = 0; i < n; ++i) {
            bs.rate[i] = requests[i].params.output_sample_rate;
            if (q3t_vocoder_stream_open(ctx_, max_len, &bs.voc[i]) != Q3T_OK || !set_stream_rate(bs.voc[i], bs.rate[i]))
                return fail_all("Failed to open the vocoder stream: " + q3t_error());
        }
    }
    const int64_t tg = now_ms();
    const int rc_gen = q3t_generate_utt(ctx_, n, tp.data(), nt.data(), spk.data(), &p, up.data(), codes.data(), nf.data(),
                                        stream_full ? batch_full_stream_cb : nullptr, &bs, stream_full ? stream_full_ : 0);
    if (rc_gen != Q3T_OK) {
        for (auto &r : out) { r.audio.clear(); r.pcm16.clear(); }
        return fail_all("Failed to generate speech codes: " + q3t_error());
    }
    if (stream_full && bs.flush()) bs.finish();   // the remainders, then the output stage's tails
    const int64_t gen_ms = now_ms() - tg - bs.decode_ms;
    for (int32_t i = 0; i < n; ++i) {
        tts_result &r = out[i];
        r.t_generate_ms = gen_ms;
        const int32_t rate = requests[i].params.output_sample_rate;
        if (nf[i] == 0) { r.error_msg = "No speech codes generated"; r.audio.clear(); r.pcm16.clear(); continue; }
        if (stream_full) {
            if (!bs.error && q3t_vocoder_stream_frames(bs.voc[i]) != nf[i])
                bs.fail("the callback saw " + std::to_string(q3t_vocoder_stream_frames(bs.voc[i])) + " of " +
                        std::to_string(nf[i]) + " generated frames");
            if (bs.error) { r.error_msg = "Vocoder stream decode failed: " + bs.error_msg; r.audio.clear(); r.pcm16.clear(); continue; }
            r.t_decode_ms = bs.decode_ms;
            r.sample_rate = rate > 0 ? rate : kSampleRate;
            r.success = true;
            continue;
        }
        const int32_t *c = codes.data() + (size_t)i * max_len * 16;
        const int64_t td = now_ms();
        if (!decode_utterance(ctx_, c, nf[i], vocoder_chunk_, rate, r)) {
            r.error_msg = "Failed to decode speech codes: " + q3t_error();
            r.audio.clear();
            r.pcm16.clear();
            continue;
        }
        r.t_decode_ms = now_ms() - td;
        r.sample_rate = rate > 0 ? rate : kSampleRate;
        r.success = true;
    }
    const int64_t total = now_ms() - t0;
    for (auto &r : out) r.t_total_ms = total;
    return out;
}

std::vector<tts_result> Qwen3TTS::synthesize_queue(const std::vector<std::string> &texts,
                                                   const std::vector<std::vector<float>> &speaker_embeddings,
                                                   const tts_params &params,
                                                   const std::function<void(int32_t, const tts_result &)> &on_result) {
    const bool bad = !speaker_embeddings.empty() && speaker_embeddings.size() != texts.size();
    return queue_requests(uniform_requests(texts, bad ? std::vector<std::vector<float>>() : speaker_embeddings, params),
                          on_result, bad ? "speaker_embeddings must be empty or hold one entry per text" : "");
}

std::vector<tts_result> Qwen3TTS::synthesize_queue(const std::vector<tts_request> &requests,
                                                   const std::function<void(int32_t, const tts_result &)> &on_result) {
    if (!models_loaded_ || !any_reference(requests)) return queue_requests(requests, on_result, "");
    // as synthesize_batch: one batched encode before the queue starts; a failed clip's request is reported at once
    std::vector<tts_request> run;
    std::vector<int32_t> index;
    std::vector<std::string> failed;
    resolve_references(requests, run, index, failed);
    std::vector<tts_result> out(requests.size());
    for (size_t i = 0; i < requests.size(); ++i) {
        if (failed[i].empty()) continue;
        out[i].error_msg = failed[i];
        if (on_result) on_result((int32_t)i, out[i]);
    }
    const std::vector<tts_result> res = queue_requests(
        run, [&](int32_t j, const tts_result &r) { if (on_result) on_result(index[j], r); }, "");
    for (size_t j = 0; j < res.size(); ++j) out[index[j]] = res[j];
    return out;
}

std::vector<tts_result> Qwen3TTS::queue_requests(const std::vector<tts_request> &requests,
                                                 const std::function<void(int32_t, const tts_result &)> &on_result,
                                                 const std::string &arg_error) {
    const int32_t n = (int32_t)requests.size();
    std::vector<tts_result> out(n);
    QueueSynthState qs;
    qs.out = &out;
    qs.on_result = &on_result;
    qs.reported.assign(n, 0);
    qs.t0 = now_ms();
    auto fail_rest = [&](const std::string &m) {   // every utterance not handed out yet ends with the error
        for (int32_t i = 0; i < n; ++i)
            if (!qs.reported[i]) qs.report(i, false, m);
        return out;
    };
    if (!models_loaded_) return fail_rest("Models not loaded");
    if (n == 0) return out;
    if (!arg_error.empty()) return fail_rest(arg_error);
    for (const tts_request &r : requests)
        if (!r.speaker_embedding.empty() && (int32_t)r.speaker_embedding.size() != hidden_)
            return fail_rest("a speaker embedding must be empty or hold one value per hidden channel");
    std::string bad_rate;
    for (const tts_request &r : requests)
        if (!rate_ok(r.params.output_sample_rate, vocoder_chunk_, bad_rate)) return fail_rest(bad_rate);
    qs.rate.resize(n);
    for (int32_t i = 0; i < n; ++i) qs.rate[i] = requests[i].params.output_sample_rate;
    std::vector<std::vector<int32_t>> toks(n);
    std::vector<const int32_t *> tp(n);
    std::vector<int32_t> nt(n), nf(n);
    const std::vector<float> zero(hidden_, 0.0f);   // no embedding: a zero speaker row, as in every call of this pipeline
    std::vector<const float *> spk(n);
    for (int32_t i = 0; i < n; ++i) {
        const int64_t t = now_ms();
        toks[i] = tokenizer_.encode_for_tts(requests[i].text);
        out[i].t_tokenize_ms = now_ms() - t;
        if (toks[i].empty()) return fail_rest("Failed to tokenize text");
        tp[i] = toks[i].data();
        nt[i] = (int32_t)toks[i].size();
        spk[i] = requests[i].speaker_embedding.empty() ? zero.data() : requests[i].speaker_embedding.data();
    }
    q3t_gen_params p;
    std::vector<q3t_utt_params> up;
    request_params(requests, seed_, p, up);
    const int32_t max_len = p.max_len;
    const int32_t slots = std::min(n, std::max(queue_slots_, 1));
    if (!ensure_slots(slots, max_len)) return fail_rest("Failed to generate speech codes: " + error_msg_);
    qs.ctx = ctx_;
    qs.stream_full = stream_full_ > 0 && vocoder_chunk_ <= 0;
    qs.vocoder_chunk = vocoder_chunk_;
    qs.max_len = max_len;
    qs.n_frames.assign(n, 0);
    qs.codes.assign(n, {});
    qs.mine.assign(n, nullptr);
    qs.decode_ms.assign(n, 0.0);
    if (qs.stream_full && !qs.open_pool(slots)) return fail_rest("Failed to open the vocoder stream: " + q3t_error());
    // the context may hold more slots than this queue uses (it only grows): max_active keeps it to `slots`
    const int rc = q3t_generate_queue_utt(ctx_, n, tp.data(), nt.data(), spk.data(), &p, up.data(), nullptr, nf.data(), slots,
                                          queue_synth_cb, &qs, qs.stream_full ? stream_full_ : kQueueTick);
    if (rc != Q3T_OK) return fail_rest("Failed to generate speech codes: " + q3t_error());
    if (!qs.error_msg.empty()) return fail_rest(qs.error_msg);
    return fail_rest("the queue ended without the utterance's final delivery");   // none is left after a clean run
}

// The open queue: requests are admitted while the others run (q3t_generate_queue_open)
bool Qwen3TTS::serve_queue(const std::function<bool(std::vector<tts_request> &, int32_t, bool)> &next_request,
                           const std::function<void(int32_t, const tts_result &)> &on_result, int32_t max_audio_tokens) {
    if (!models_loaded_) { error_msg_ = "Models not loaded"; return false; }
    if (!next_request) { error_msg_ = "serve_queue: no request source"; return false; }
    const int32_t slots = std::max(queue_slots_, 1), max_len = std::max(max_audio_tokens, 1);
    if (!ensure_slots(slots, max_len)) return false;
    OpenQueueState qs;
    qs.ctx = ctx_;
    qs.stream_full = stream_full_ > 0 && vocoder_chunk_ <= 0;
    qs.vocoder_chunk = vocoder_chunk_;
    qs.max_len = max_len;
    qs.hidden = hidden_;
    qs.tokenizer = &tokenizer_;
    qs.next_request = &next_request;
    qs.on_result = &on_result;
    qs.encode_speakers = [this](const std::vector<std::string> &paths, std::vector<std::vector<float>> &emb,
                                std::vector<std::string> &err) { return encode_speakers(paths, emb, err); };
    qs.zero.assign(hidden_, 0.0f);   // no embedding: a zero speaker row, as in every call of this pipeline
    q3t_default_params(&qs.p);
    qs.p.seed = seed_;
    qs.p.max_len = max_len;
    if (qs.stream_full && !qs.open_pool(slots)) { error_msg_ = "Failed to open the vocoder stream: " + q3t_error(); return false; }
    // (the context may hold more slots than this queue uses: it only grows)
    const int rc = q3t_generate_queue_open(ctx_, &qs.p, slots, slots, open_queue_arrive, open_queue_cb, &qs,
                                           qs.stream_full ? stream_full_ : kQueueTick, nullptr, nullptr);
    const std::string why = rc != Q3T_OK ? "Failed to generate speech codes: " + q3t_error()
                            : !qs.error_msg.empty() ? qs.error_msg : "the queue ended without the utterance's final delivery";
    for (auto &kv : qs.live) qs.report(kv.second, false, why);   // none is left after a clean run
    if (rc == Q3T_OK && qs.error_msg.empty()) return true;
    error_msg_ = why;
    return false;
}

// ======================================================================================================= audio

void resample_linear(const float *input, int input_len, int input_rate, std::vector<float> &output, int output_rate) {
    const double ratio = (double)input_rate / output_rate;
    const int out_len = (int)((double)input_len / ratio);
    output.resize(std::max(out_len, 0));
    for (int i = 0; i < out_len; ++i) {
        const double src = i * ratio;
        const int i0 = (int)src, i1 = i0 + 1;
        const double frac = src - i0;
        output[i] = i1 >= input_len ? input[input_len - 1] : (float)((1.0 - frac) * input[i0] + frac * input[i1]);
    }
}

bool load_audio_file(const std::string &path, std::vector<float> &samples, int &sample_rate) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "ERROR: Cannot open WAV file: %s\n", path.c_str()); return false; }
    auto done = [&](bool ok) { fclose(f); return ok; };
    char tag[4];
    uint32_t u32 = 0;
    if (fread(tag, 1, 4, f) != 4 || memcmp(tag, "RIFF", 4) != 0) { fprintf(stderr, "ERROR: Not a RIFF file\n"); return done(false); }
    if (fread(&u32, 4, 1, f) != 1) return done(false);
    if (fread(tag, 1, 4, f) != 4 || memcmp(tag, "WAVE", 4) != 0) { fprintf(stderr, "ERROR: Not a WAVE file\n"); return done(false); }
    uint16_t fmt = 0, ch = 0, bits = 0;
    uint32_t sr = 0;
    for (;;) {
        uint32_t size = 0;
        if (fread(tag, 1, 4, f) != 4 || fread(&size, 4, 1, f) != 1) break;
        if (memcmp(tag, "fmt ", 4) == 0) {
            if (fread(&fmt, 2, 1, f) != 1 || fread(&ch, 2, 1, f) != 1 || fread(&sr, 4, 1, f) != 1) break;
            fseek(f, 6, SEEK_CUR);   // byte rate + block align
            if (fread(&bits, 2, 1, f) != 1) break;
            if (size > 16) fseek(f, size - 16, SEEK_CUR);
        } else if (memcmp(tag, "data", 4) == 0) {
            sample_rate = (int)sr;
            if (ch == 0) return done(false);
            const int width = (fmt == 1 && bits == 16) ? 2 : ((fmt == 1 && bits == 32) || fmt == 3) ? 4 : 0;
            if (width == 0) {
                if (fmt == 1) fprintf(stderr, "ERROR: Unsupported bits per sample: %d\n", bits);
                else fprintf(stderr, "ERROR: Unsupported audio format: %d\n", fmt);
                return done(false);
            }
            const size_t n = size / ((size_t)width * ch);
            std::vector<uint8_t> raw(n * ch * width);
            if (fread(raw.data(), (size_t)width, n * ch, f) != n * ch) return done(false);
            samples.resize(n);
            for (size_t i = 0; i < n; ++i) {
                float sum = 0.0f;
                for (int c = 0; c < ch; ++c) {
                    const uint8_t *p = raw.data() + (i * ch + c) * width;
                    if (width == 2) { int16_t v; memcpy(&v, p, 2); sum += v / 32768.0f; }
                    else if (fmt == 1) { int32_t v; memcpy(&v, p, 4); sum += v / 2147483648.0f; }
                    else { float v; memcpy(&v, p, 4); sum += v; }
                }
                samples[i] = sum / ch;
            }
            return done(true);
        } else {
            fseek(f, size, SEEK_CUR);
        }
    }
    fprintf(stderr, "ERROR: No data chunk found\n");
    return done(false);
}

bool save_audio_file(const std::string &path, const std::vector<float> &samples, int sample_rate) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "ERROR: Cannot create WAV file: %s\n", path.c_str()); return false; }
    const uint16_t ch = 1, bits = 16, block = ch * bits / 8, fmt = 1;
    const uint32_t sr = (uint32_t)sample_rate, byte_rate = sr * block, data = (uint32_t)(samples.size() * block);
    const uint32_t riff = 36 + data, fmt_size = 16;
    std::vector<uint8_t> h;
    auto put = [&](const void *p, size_t n) { h.insert(h.end(), (const uint8_t *)p, (const uint8_t *)p + n); };
    put("RIFF", 4); put(&riff, 4); put("WAVE", 4);
    put("fmt ", 4); put(&fmt_size, 4); put(&fmt, 2); put(&ch, 2); put(&sr, 4); put(&byte_rate, 4); put(&block, 2);
    put(&bits, 2);
    put("data", 4); put(&data, 4);
    std::vector<int16_t> pcm(samples.size());
    for (size_t i = 0; i < samples.size(); ++i) {
        const float s = std::min(1.0f, std::max(-1.0f, samples[i]));
        pcm[i] = (int16_t)(s * 32767.0f);   // truncation toward zero, as the reference's cast
    }
    const bool ok = fwrite(h.data(), 1, h.size(), f) == h.size() &&
                    (pcm.empty() || fwrite(pcm.data(), 2, pcm.size(), f) == pcm.size());
    fclose(f);
    return ok;
}

bool save_audio_file(const std::string &path, const std::vector<int16_t> &pcm, int sample_rate) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "ERROR: Cannot create WAV file: %s\n", path.c_str()); return false; }
    const uint16_t ch = 1, bits = 16, block = ch * bits / 8, fmt = 1;
    const uint32_t sr = (uint32_t)sample_rate, byte_rate = sr * block, data = (uint32_t)(pcm.size() * block);
    const uint32_t riff = 36 + data, fmt_size = 16;
    std::vector<uint8_t> h;
    auto put = [&](const void *p, size_t n) { h.insert(h.end(), (const uint8_t *)p, (const uint8_t *)p + n); };
    put("RIFF", 4); put(&riff, 4); put("WAVE", 4);
    put("fmt ", 4); put(&fmt_size, 4); put(&fmt, 2); put(&ch, 2); put(&sr, 4); put(&byte_rate, 4); put(&block, 2);
    put(&bits, 2);
    put("data", 4); put(&data, 4);
    const bool ok = fwrite(h.data(), 1, h.size(), f) == h.size() &&
                    (pcm.empty() || fwrite(pcm.data(), 2, pcm.size(), f) == pcm.size());
    fclose(f);
    return ok;
}

bool save_audio_file(const std::string &path, const tts_result &r) {
    return r.pcm16.empty() ? save_audio_file(path, r.audio, r.sample_rate) : save_audio_file(path, r.pcm16, r.sample_rate);
}

}  // namespace qwen3_tts
