// qwen3_tts_pipeline.h — the reference's pipeline surface (src/qwen3_tts.h:17-156): tts_params, tts_result, Qwen3TTS,
// load_audio_file, save_audio_file, over the component classes of qwen3_tts_hip.h.  Same names, fields, defaults and
// error convention; the deliberate differences are listed in qwen3_tts_hip.h.  Library: libqwen3_tts_pipeline.so.
#ifndef QWEN3_TTS_PIPELINE_H
#define QWEN3_TTS_PIPELINE_H

#include <functional>
#include <memory>

#include "qwen3_tts_hip.h"

namespace qwen3_tts {

// ====================================================================================== pipeline (src/qwen3_tts.h)
struct tts_params {
    int32_t max_audio_tokens = 4096;
    float temperature = 0.9f;
    float top_p = 1.0f;       // accepted, unused (as in the reference: no top-p stage exists in its sampler)
    int32_t top_k = 50;
    int32_t n_threads = 4;    // accepted, unused (host threads do no numeric work here)
    bool print_progress = false;
    bool print_timing = true;
    float repetition_penalty = 1.05f;
    // MI355X extension.  0: float32 at 24 kHz in tts_result::audio, as the reference.  One of 8000, 12000, 16000,
    // 22050, 24000, 32000, 44100, 48000: the device's output stage (q3t_vocoder_decode_out / _stream_push_out /
    // _stream_push_batch_out) delivers s16 at that rate in tts_result::pcm16 and audio stays empty; no host
    // conversion runs.  Needs the whole-utterance vocoder (vocoder_chunk() == 0); in a tts_request it is the
    // request's own
    int32_t output_sample_rate = 0;
};

struct tts_result {
    std::vector<float> audio;
    int32_t sample_rate = 24000;      // the delivered rate: tts_params::output_sample_rate when one was asked for
    std::vector<int16_t> pcm16;       // the device s16 stream at sample_rate, in place of audio, when one was asked for
    size_t num_samples() const { return pcm16.empty() ? audio.size() : pcm16.size(); }
    bool success = false;
    std::string error_msg;
    int64_t t_load_ms = 0;
    int64_t t_tokenize_ms = 0;
    int64_t t_encode_ms = 0;
    int64_t t_generate_ms = 0;
    int64_t t_decode_ms = 0;
    int64_t t_total_ms = 0;
    uint64_t mem_rss_start_bytes = 0;
    uint64_t mem_rss_end_bytes = 0;
    uint64_t mem_rss_peak_bytes = 0;
    uint64_t mem_phys_start_bytes = 0;
    uint64_t mem_phys_end_bytes = 0;
    uint64_t mem_phys_peak_bytes = 0;
};

// one utterance of a mixed batch or queue (synthesize_batch / synthesize_queue over requests): its own text, voice
// (empty: a zero speaker row, as in every call of this pipeline), sampling values, max_audio_tokens and language.  What stays per call: the seed
// (set_seed) and the reporting switches of tts_params (print_progress / print_timing are not used by these calls).
struct tts_request {
    std::string text;
    std::vector<float> speaker_embedding;
    // the voice as a reference clip (a WAV file) instead: resampled and encoded like synthesize_with_voice's, through
    // the voice cache, the clips of one call in one batched encode (Qwen3TTS::encode_speakers).  Empty changes
    // nothing; giving both it and speaker_embedding is a check_request error
    std::string reference_audio;
    tts_params params;
    int32_t language_id = 2050;   // < 0: the nothink prompt
};

class VoiceCache;

class Qwen3TTS {
public:
    Qwen3TTS();
    ~Qwen3TTS();
    Qwen3TTS(const Qwen3TTS &) = delete;
    Qwen3TTS &operator=(const Qwen3TTS &) = delete;

    // model_dir holds qwen3-tts-0.6b-f16.gguf and qwen3-tts-tokenizer-f16.gguf (qwen3_tts.cpp:117-118)
    bool load_models(const std::string &model_dir);
    tts_result synthesize(const std::string &text, const tts_params &params = tts_params());
    tts_result synthesize_with_voice(const std::string &text, const std::string &reference_audio,
                                     const tts_params &params = tts_params());
    tts_result synthesize_with_voice(const std::string &text, const float *ref_samples, int32_t n_ref_samples,
                                     const tts_params &params = tts_params());
    bool encode_speaker(const std::string &reference_audio, std::vector<float> &embedding);
    // MI355X extension: many reference clips at once.  embeddings[i] / errors[i] for reference_audios[i] (errors[i]
    // empty: embeddings[i] holds the voice, bit for bit encode_speaker's).  The voices met before come from a bounded
    // LRU cache keyed by (path, file size, modification time) (voice_cache.h, 64 entries); the others are loaded,
    // resampled to 24 kHz as encode_speaker does, and encoded in ONE q3t_speaker_encode_batch call.  A clip that cannot
    // be read or is too short fails alone.  False with get_error(): nothing could run (no models, no speaker encoder)
    bool encode_speakers(const std::vector<std::string> &reference_audios, std::vector<std::vector<float>> &embeddings,
                         std::vector<std::string> &errors);
    tts_result synthesize_with_embedding(const std::string &text, const std::vector<float> &speaker_embedding,
                                         const tts_params &params = tts_params());
    const std::string &get_error() const { return error_msg_; }
    bool is_loaded() const { return models_loaded_; }

    // ---- MI355X extensions
    bool set_device(int device);           // before load_models
    void set_seed(uint64_t seed) { seed_ = seed; }
    // 0: whole-utterance vocoder after generation; n > 0: n-frame chunks streamed from the frame callback
    void set_vocoder_chunk(int32_t frames) { vocoder_chunk_ = frames; }
    int32_t vocoder_chunk() const { return vocoder_chunk_; }
    // n > 0 (and no chunked vocoder): synthesize() generates through the frame callback every n frames and pushes
    // each delivery into a vocoder stream (q3t_vocoder_stream_*): the whole-utterance vocoder's PCM, bit for bit,
    // produced while the frames are generated.  synthesize_batch() does the same with one stream per utterance, the
    // deliveries of one interval pushed together (q3t_vocoder_stream_push_batch).  0 (default): whole-utterance
    // vocoder after generation
    void set_stream_full(int32_t interval) { stream_full_ = interval; }
    int32_t stream_full() const { return stream_full_; }
    // n utterances decoded together on one GPU (lock-step slots); speaker_embeddings empty or one per text (an empty
    // vector = no speaker row); results[i] as synthesize_with_embedding's
    std::vector<tts_result> synthesize_batch(const std::vector<std::string> &texts,
                                             const std::vector<std::vector<float>> &speaker_embeddings,
                                             const tts_params &params = tts_params());
    // the same with every utterance's own voice, language, sampling values and max_audio_tokens (q3t_generate_utt);
    // the overload above forwards here with one tts_params for all.  The reference clips of the call are resolved in
    // one encode_speakers call before generating; a request whose clip fails gets a failed result with that message
    // and the rest run (synthesize_queue over requests does the same)
    std::vector<tts_result> synthesize_batch(const std::vector<tts_request> &requests);

    // false with the reason when the engine would refuse this request's values (language id at or above the codec
    // vocabulary, top_k < 0, a repetition penalty that is not finite and > 0, a temperature that is not finite, an
    // embedding of the wrong length, an output_sample_rate the output stage does not have or one beside a chunked vocoder): such a request fails the whole synthesize_batch / synthesize_queue call it is
    // part of, so a server checks each request first and answers it alone.  max_audio_tokens needs no check: the
    // context grows to the longest request
    bool check_request(const tts_request &request, std::string &error) const;

    // Continuous batching (q3t_generate_queue_stream): any number of texts through set_queue_slots(n) slots, a slot
    // refilled with the next text when its utterance ends.  on_result(index, result) fires at the utterance's final
    // delivery, while the others still run, so results come in completion order; the returned vector holds them in
    // text order.  With set_stream_full(n) every running utterance holds one vocoder stream of a pool of one per slot,
    // opened before the queue starts (reset when the next utterance takes it), and each delivery callback makes one
    // q3t_vocoder_stream_push_batch over its pieces; without it an utterance is decoded whole (or in
    // vocoder_chunk() chunks) at its final delivery.  The audio equals synthesize_with_embedding's vocoder output of
    // the queue's codes.  t_decode_ms is the utterance's share (by frames) of the batched pushes, or its own decode;
    // t_generate_ms the rest of its time since the call began, the wait for a slot included.  An error ends the
    // queue: every utterance not handed out yet gets the message.
    void set_queue_slots(int32_t slots) { queue_slots_ = slots; }
    int32_t queue_slots() const { return queue_slots_; }
    std::vector<tts_result> synthesize_queue(const std::vector<std::string> &texts,
                                             const std::vector<std::vector<float>> &speaker_embeddings,
                                             const tts_params &params = tts_params(),
                                             const std::function<void(int32_t, const tts_result &)> &on_result = nullptr);
    // the same over requests (q3t_generate_queue_utt): requests that differ in voice, language, sampling values or
    // max_audio_tokens share the slots.  The overload above forwards here
    std::vector<tts_result> synthesize_queue(const std::vector<tts_request> &requests,
                                             const std::function<void(int32_t, const tts_result &)> &on_result = nullptr);

    // The open queue (q3t_generate_queue_open): requests are taken while the others run, so one that arrives a frame
    // after the call began is admitted into a free slot at once instead of waiting for the queue to drain.
    // next_request(out, room, may_block) is asked between two frames whenever a slot could take a newcomer: it appends
    // at most `room` requests to `out` and returns false when no more will come (the call returns when the accepted
    // ones have ended).  It must return at once unless may_block is true (nothing runs: it may wait for a request).
    // Requests are numbered from 0 in the order they are handed over; on_result(number, result) fires at a request's
    // final delivery, or at once, alone, for one that is refused (the checks of check_request and of the engine, a text
    // that does not tokenize, more max_audio_tokens than the call's).  max_audio_tokens is the cap of every request of
    // the call: the context is sized once, before the first request.  Reference clips (tts_request::reference_audio)
    // are resolved on the calling thread, between two frames, for exactly the requests about to be handed to the
    // engine, in one encode_speakers call; a request whose clip fails is refused.  Slots, vocoder handling and timings are
    // synthesize_queue's; a request's codes are those synthesize_queue gives it at the index it has among the accepted
    // requests.  The device lock of the context is held for the whole call, also while next_request blocks.  False with
    // get_error(): an engine error ended the call (every running request got the message).
    bool serve_queue(const std::function<bool(std::vector<tts_request> &, int32_t, bool)> &next_request,
                     const std::function<void(int32_t, const tts_result &)> &on_result, int32_t max_audio_tokens = 4096);

private:
    tts_result synthesize_internal(const std::string &text, const float *speaker_embedding, const tts_params &params,
                                   tts_result &result);
    bool ensure_slots(int32_t slots, int32_t max_len);
    // the requests of a closed-set call with their references resolved (run: the ones to generate, index: their
    // places in `requests`); failed[i] non-empty: request i's clip failed, or it gives a clip and an embedding
    void resolve_references(const std::vector<tts_request> &requests, std::vector<tts_request> &run,
                            std::vector<int32_t> &index, std::vector<std::string> &failed);
    std::vector<tts_result> batch_requests(const std::vector<tts_request> &requests, const std::string &arg_error);
    std::vector<tts_result> queue_requests(const std::vector<tts_request> &requests,
                                           const std::function<void(int32_t, const tts_result &)> &on_result,
                                           const std::string &arg_error);

    TextTokenizer tokenizer_;
    std::unique_ptr<VoiceCache> voices_;
    q3t_ctx *ctx_ = nullptr;
    int device_ = 0;
    uint64_t seed_ = 0;
    int32_t slots_ = 0, n_ctx_ = 0, hidden_ = 1024, codec_vocab_ = 3072;
    int32_t vocoder_chunk_ = 0;
    int32_t stream_full_ = 0;
    int32_t queue_slots_ = 1;
    bool models_loaded_ = false;
    std::string error_msg_;
    std::string tts_model_path_;
    std::string decoder_model_path_;
};

// WAV: RIFF PCM16 / PCM32 / IEEE float32, channels averaged to mono (qwen3_tts.cpp:567-706)
bool load_audio_file(const std::string &path, std::vector<float> &samples, int &sample_rate);
// WAV PCM16 mono, samples clamped to [-1, 1] and scaled by 32767 (qwen3_tts.cpp:708-759)
bool save_audio_file(const std::string &path, const std::vector<float> &samples, int sample_rate);
// the same file from s16 samples as they are (the output stage's): no conversion
bool save_audio_file(const std::string &path, const std::vector<int16_t> &samples, int sample_rate);
// the result's WAV: pcm16 as it is when the request asked for a sample rate, else audio through the conversion above
bool save_audio_file(const std::string &path, const tts_result &result);
// linear resampling used for reference audio (qwen3_tts.cpp:83-101)
void resample_linear(const float *input, int input_len, int input_rate, std::vector<float> &output, int output_rate);

}  // namespace qwen3_tts

#endif
