/* q3t_backend.h — C ABI of the MI355X-native Qwen3-TTS decode path (libq3t.so).
 *
 * Plain pointers and sizes only; every call returns Q3T_OK (0) or Q3T_ERR (-1) and leaves a message in the
 * thread-local q3t_last_error() (the reference's `bool` + get_error() convention, src/tts_transformer.h:244,
 * src/trt_code_predictor.h:85).  One q3t_ctx per GPU; calls on one context are not thread-safe, contexts on
 * different devices may be driven by different host threads.  All buffers below are HOST buffers unless the
 * name says _dev; the hot path keeps everything resident in HBM between calls.
 *
 * Interfaces replaced (reference file:line):
 *   q3t_ctx_create        TTSTransformer::load_model (src/tts_transformer.h:170, .cpp:51) +
 *                         AudioTokenizerDecoder::load_model (src/audio_tokenizer_decoder.h:165) +
 *                         TRTCodePredictor::load_engine/upload_* (src/trt_code_predictor.h:31-50)
 *   q3t_generate          TTSTransformer::generate (src/tts_transformer.h:233-241, .cpp:2342-2574)
 *   q3t_generate_stream   the same with frame_callback_t on_frames / callback_interval (src/tts_transformer.h:224,
 *                         .cpp:2517-2523, 2563-2570; caller qwen3_tts.cpp:437-463: the TRT streaming vocoder)
 *   q3t_generate_queue    continuous batching over the same path (no reference counterpart: SURVEY §7 step 9,
 *                         the serving extension of TTSTransformer::generate to more utterances than slots)
 *   q3t_comm_unique_id,   SURVEY §8(e) multi-GPU start-up (no reference counterpart: the reference is one process
 *   q3t_ctx_create_shared on one Jetson): RCCL broadcast of rank 0's packed weight blobs over xGMI
 *   q3t_ctx_create_replica, q3t_comm_allreduce_max
 *   q3t_talker_forward    TTSTransformer::forward_step (src/tts_transformer.h:189-192, .cpp:1952-2028)
 *   q3t_talker_prefill    TTSTransformer::forward_prefill (src/tts_transformer.h:196-198, .cpp:1233-1374, 1829-1920)
 *   q3t_codepred_frame    TTSTransformer::predict_codes_autoregressive (src/tts_transformer.h:203-207) /
 *                         TRTCodePredictor::run_greedy_loop / run_sampling_loop (src/trt_code_predictor.h:68-79)
 *   q3t_cb0_select        CB0 logit processing inside generate (src/tts_transformer.cpp:2417-2499)
 *   q3t_project_text      TTSTransformer::project_text_tokens (src/tts_transformer.cpp:1026-1091)
 *   q3t_prefill_embd      TTSTransformer::build_prefill_graph (src/tts_transformer.cpp:1093-1231)
 *   q3t_vocoder_decode    AudioTokenizerDecoder::decode (src/audio_tokenizer_decoder.h:173-174) [FULL] and
 *                         TRTVocoderDecoder::decode (src/trt_vocoder.h:33-34) [CHUNK40]
 *   gpu_*                 the four extern "C" wrappers of src/trt_cuda_kernels.cu:10,60,78,183
 */
#ifndef Q3T_BACKEND_H
#define Q3T_BACKEND_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Q3T_OK 0
#define Q3T_ERR (-1)
#define Q3T_VOCODER_FULL 0    /* whole utterance, GGML decoder semantics */
#define Q3T_VOCODER_CHUNK40 1 /* independent 40-frame chunks, 1920 samples/frame (TRT streaming) */

typedef struct q3t_ctx q3t_ctx;

typedef struct q3t_config {
    int32_t hidden, n_layers, n_heads, n_kv_heads, head_dim, intermediate;
    int32_t codec_vocab, n_codebooks, text_vocab, text_dim, cp_layers, cp_vocab;
    int32_t codec_eos, has_vocoder, sample_rate, max_slots, max_ctx;
    /* code predictor geometry (tts_transformer.cpp:370-389): equal to the talker's for 0.6B; 1.7B projects every
     * code-predictor input with code_pred.mtp_proj (has_mtp = 1) */
    int32_t cp_hidden, cp_intermediate, cp_heads, cp_kv_heads, has_mtp;
} q3t_config;

/* tts_params (src/qwen3_tts.h:18-43) + generate() arguments; top_p / n_threads are unused by the reference */
typedef struct q3t_gen_params {
    int32_t max_len;            /* max_audio_tokens (frames), default 4096 */
    int32_t language_id;        /* 2050 (english) as passed by synthesize_internal, qwen3_tts.cpp:459-463 */
    float repetition_penalty;   /* 1.05 */
    float temperature;          /* 0.9; <= 0 => greedy */
    int32_t top_k;              /* 50 */
    uint64_t seed;              /* counter-based sampler seed (the reference seeds std::mt19937 from random_device) */
    int32_t force_frames;       /* bench only: EOS masked until this many frames (0 = off) */
} q3t_gen_params;

const char *q3t_last_error(void);
void q3t_default_params(q3t_gen_params *p);

/* tts_gguf may be NULL: a vocoder-only context (AudioTokenizerDecoder::load_model / TRTVocoderDecoder::load_engine
 * without a talker); the talker entry points then fail with an error.  tokenizer_gguf may be NULL: no vocoder. */
int q3t_ctx_create(const char *tts_gguf, const char *tokenizer_gguf /* may be NULL: no vocoder */, int device,
                   int max_slots, int max_ctx, q3t_ctx **out);
void q3t_ctx_destroy(q3t_ctx *ctx);

/* ---- multi-GPU (one process per GPU): rank 0 calls q3t_comm_unique_id and hands the bytes to the other ranks by any
 * host channel; every rank then calls q3t_ctx_create_shared.  Only rank 0 reads tensor bytes from the GGUF files; the
 * other ranks parse the headers, lay out identical weight blobs and receive them by ncclBroadcast (RCCL over xGMI). */
#define Q3T_COMM_ID_BYTES 128
int q3t_comm_unique_id(uint8_t *id /* [Q3T_COMM_ID_BYTES] */);
int q3t_ctx_create_shared(const char *tts_gguf, const char *tokenizer_gguf, int device, int max_slots, int max_ctx,
                          int rank, int world, const uint8_t *id, q3t_ctx **out);
/* host-only weight layout of a model file (no device touched): the byte offset of every allocation of the talker blob
 * in order (n_alloc of them; offsets may be NULL to query n_alloc, else max_n entries) and the bytes used -- what every
 * rank of q3t_ctx_create_shared computes from the GGUF headers before the broadcast (whose size check compares
 * `used` across ranks) */
int q3t_plan_weight_layout(const char *tts_gguf, uint64_t *offsets, int max_n, int *n_alloc, uint64_t *used);
/* a second context whose weight blobs are copied device-to-device from src's (same or peer device, no file reads) */
int q3t_ctx_create_replica(q3t_ctx *src, int device, int max_slots, int max_ctx, q3t_ctx **out);
/* element-wise max over the ranks of a shared context (n <= 64 host doubles; also a barrier); no-op otherwise */
int q3t_comm_allreduce_max(q3t_ctx *ctx, double *values, int n);
int q3t_get_config(const q3t_ctx *ctx, q3t_config *out);

/* ---- hot path: prefill + frame loop for n_utt utterances batched in lock-step.
 * tokens[u] -> n_tokens[u] chat-template ids; speaker[u] -> hidden floats or speaker == NULL (all or none).
 * codes: [n_utt][p->max_len][16] int32 row-major [frame][codebook]; n_frames[u] = frames produced. */
int q3t_generate(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens,
                 const float *const *speaker, const q3t_gen_params *p, int32_t *codes, int32_t *n_frames);
/* streaming: on_frames(user, u, codes [n][16], n, 16) is called on the caller's thread every `interval` frames of
 * utterance u with its newest `interval` frames, and once more after the loop with the remainder (< interval
 * frames, or the frames before EOS); returning 0 stops utterance u after the frames delivered so far.  The callback
 * may call q3t_vocoder_decode on the same context (it runs behind the frames already queued).  The callback runs
 * while the generate holds its device lock (shared for batches, exclusive for one utterance): it must not start a
 * one-utterance generate on another context of the same device, and a wait in it for another thread's work on the
 * same device can be delayed up to 20 ms by a one-utterance generate queued meanwhile (devlock.h). */
typedef int (*q3t_frame_cb)(void *user, int32_t utterance, const int32_t *codes, int32_t n_frames, int32_t n_codebooks);
int q3t_generate_stream(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens,
                        const float *const *speaker, const q3t_gen_params *p, int32_t *codes, int32_t *n_frames,
                        q3t_frame_cb on_frames, void *user, int32_t interval);
/* continuous batching: n_utt utterances (any number; codes [n_utt][max_len][16], n_frames [n_utt]) through
 * min(max_slots, n_utt) slots with at most max_active (<= 0: all slots) in flight.  When an utterance ends (EOS or
 * max_len) its slot is refilled with the next one between two frames (prefill of the newcomer on that slot only).
 * Sampling is keyed by the utterance's index in the call, so an utterance's codes do not depend on its slot, on when
 * it was admitted or on its neighbours.  A newcomer's prefill runs on its own stream, overlapping the other slots'
 * decoding, with the batch's kernels (>= 4 slots: the first wave's codes equal q3t_generate's). */
int q3t_generate_queue(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens,
                       const float *const *speaker, const q3t_gen_params *p, int32_t *codes, int32_t *n_frames,
                       int32_t max_active);
/* q3t_generate_queue that hands frames out while it runs, reports an utterance when it ends and lets the caller cancel
 * one.  Every `interval` frames of the queue's frame loop (a tick) the new frames of all running utterances are
 * collected by one launch and one copy; when utterances end (EOS or max_len) the rest of their frames are collected
 * the same way and marked final, before their slots are refilled.
 * one call per tick or finish: n entries; utt[i] = utterance index in the call, codes[i] -> [n_frames[i]][16] (valid during
 * the call only), final[i] != 0 on the utterance's last delivery; stop[i] (zeroed by the caller of the callback) set
 * non-zero cancels utt[i].  Entries come in increasing utt[i].  Return 0 to abort the whole queue.
 * Per utterance: deliveries arrive in order; a non-final one carries 1..interval frames; there is exactly one final
 * one, of 0..interval frames; their concatenation is, bit for bit and in length, what q3t_generate_queue returns for the
 * utterance (the EOS frame excluded); a delivery that is not the utterance's first and does not complete it has exactly
 * `interval` frames.  A delivery is made one tick late (a final one a frame late), so the device keeps running during
 * the callback.  A cancelled utterance gets no further delivery, n_frames[u] = the frames it was handed, and its slot
 * is refilled like a finished one; the other utterances' codes do not change (sampling is keyed by the utterance index).
 * After an abort the call returns Q3T_OK with every n_frames[u] = the frames handed out.
 * codes may be NULL: the per-utterance device copies (n_utt x max_len x 64 bytes) and the end-of-call copy are skipped.
 * cb == NULL or interval <= 0: Q3T_ERR (use q3t_generate_queue).
 * The callback runs on the caller's thread while the call holds its device lock.  It may call q3t_vocoder_stream_push,
 * q3t_vocoder_stream_push_batch, q3t_vocoder_stream_reset and q3t_vocoder_decode on the same context, under the rule
 * stated for q3t_generate_stream: they run behind the frames already queued; the callback must not start a
 * one-utterance generate on another context of the same device, and a wait in it for another thread's work on the same
 * device can be delayed up to 20 ms by a one-utterance generate queued meanwhile (devlock.h). */
typedef int (*q3t_queue_cb)(void *user, int32_t n, const int32_t *utt, const int32_t *const *codes,
                            const int32_t *n_frames, const int32_t *final, int32_t *stop);
int q3t_generate_queue_stream(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens,
                              const float *const *speaker, const q3t_gen_params *p, int32_t *codes /* may be NULL */,
                              int32_t *n_frames, int32_t max_active, q3t_queue_cb cb, void *user, int32_t interval);
/* ---- per-utterance language, speaker, sampling and max_len.  One record per utterance replaces the call-wide values
 * of q3t_gen_params, so requests that differ in any of them share one batch or one queue.  What stays per call: the
 * seed and p->max_len, the stride of `codes` ([n_utt][p->max_len][16]) and the cap of every record's max_len. */
typedef struct q3t_utt_params {
    int32_t language_id;        /* as in q3t_gen_params; < 0: the nothink prompt (one row shorter) */
    int32_t max_len;            /* 1 .. p->max_len; <= 0: p->max_len */
    float repetition_penalty;
    float temperature;          /* <= 0: greedy */
    int32_t top_k;
    int32_t force_frames;
} q3t_utt_params;
/* the call-wide values of p as one record */
void q3t_utt_params_from(const q3t_gen_params *p, q3t_utt_params *out);
/* q3t_generate / q3t_generate_stream (on_frames == NULL: no streaming) and q3t_generate_queue / q3t_generate_queue_stream
 * (cb == NULL: no deliveries; codes may be NULL only with a callback) with up[u] for utterance u.  p gives max_len and
 * seed only; its other fields are ignored.  speaker[u] may be NULL for any subset of the utterances (speaker == NULL:
 * none).  Sampling stays keyed by (seed, utterance index or slot, frame, step), so an utterance's codes are those of a
 * call in which every utterance has its values, and a smaller max_len gives a prefix of the longer run.
 * n_frames[u] <= up[u].max_len, and no callback hands out a frame at or beyond an utterance's own max_len; rows of
 * codes at or beyond it are not written by q3t_generate_utt.  Everything else is as stated for the counterparts above
 * (callback rules, the delivery contract, cancel and abort).
 * Every record is validated before anything runs; Q3T_ERR with a message naming the utterance, no state changed and
 * every n_frames[u] = 0: language_id >= codec_vocab, max_len > p->max_len, prompt length + its max_len + 8 > max_ctx,
 * top_k < 0, repetition_penalty <= 0 or not finite, temperature not finite.
 * Batches of two or more slots read each slot's sampling values from a device record; a one-slot context bakes them
 * into its captured graphs and captures again when they change between utterances. */
int q3t_generate_utt(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens,
                     const float *const *speaker, const q3t_gen_params *p, const q3t_utt_params *up /* [n_utt] */,
                     int32_t *codes, int32_t *n_frames, q3t_frame_cb on_frames, void *user, int32_t interval);
int q3t_generate_queue_utt(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens,
                           const float *const *speaker, const q3t_gen_params *p, const q3t_utt_params *up /* [n_utt] */,
                           int32_t *codes, int32_t *n_frames, int32_t max_active, q3t_queue_cb cb, void *user,
                           int32_t interval);
/* ---- incremental text input: feed an utterance's text while it speaks.  The prefill holds only the role ids and the
 * first text id; every later text id is consumed one per frame, so frame f needs text row f and nothing beyond it.
 * An utterance with open[u] != 0 is given as a head: tokens[u] = the three role ids, then >= 1 text id (n_tokens[u] >= 4),
 * WITHOUT the five-id suffix of a whole prompt.  Its further text ids come from text_cb.  With K = the text ids known
 * beyond the first (n_tokens[u] - 4 plus the ids fed so far) it may run frame f only while f < K; a slot that has
 * consumed every row it knows is put on hold (no selection, no advance, its state kept) until text_cb gives more or
 * ends the text.  The codes and n_frames of an open utterance are, bit for bit, those q3t_generate_queue_utt gives for
 * the prompt head || fed ids || five valid ids (same seed, utterance index, slot count and record), however the ids
 * were cut into feeds and however long the slot was starved; closed utterances of the call are not affected.
 *
 * asked for more text of open utterance `utt`: frames = frames it has generated, rows_ahead = frames it can still
 * run before it is held.  *ids -> *n_ids text ids (valid until return; may be 0), *end != 0: the text ends after them.
 * Return 0 to abort the whole queue (as q3t_queue_cb). */
typedef int (*q3t_text_cb)(void *user, int32_t utt, int32_t frames, int32_t rows_ahead,
                           const int32_t **ids, int32_t *n_ids, int32_t *end);
/* q3t_generate_queue_utt (up == NULL: q3t_generate_queue / q3t_generate_queue_stream) with open utterances.  text_cb
 * runs on the caller's thread under the rules stated for q3t_queue_cb, for every open utterance that holds a slot: once
 * when it is activated (before its first frame), at every tick (every `interval` frames of the loop clock) and on every
 * loop iteration on which it has no row for its next frame.  interval > 0 is required also with cb == NULL.  While every
 * busy slot is held and no admission is in flight the loop launches nothing, hands out the pending deliveries and keeps
 * asking: blocking until text exists is the callback's job.  On a fallback re-run (a persistent hand-off fault) the ids
 * already given are replayed, not asked for again; held[u] may then differ, the codes may not.
 * Deliveries of an open utterance (also after its text ended): a delivery that is neither first nor last has
 * 1..interval frames, and a tick that finds no new frame makes none; every other clause of the delivery contract holds,
 * and closed utterances keep all of it.  text_cb returning 0 with cb == NULL: utterances that had ended keep their
 * frames, the others have n_frames 0.
 * Q3T_ERR before anything runs: open != NULL with an open utterance and text_cb == NULL, interval <= 0, a head shorter
 * than 4 ids, a head id out of range.  Q3T_ERR naming the utterance, after both streams are drained: a fed id out of
 * range, a feed that takes K + 1 past the trailing-text buffer (512 rows).
 * open == NULL or all zero: the call is q3t_generate_queue_utt, launch for launch. */
int q3t_generate_queue_text(q3t_ctx *ctx, int n_utt, const int32_t *const *tokens, const int32_t *n_tokens,
                            const float *const *speaker, const q3t_gen_params *p, const q3t_utt_params *up /* may be NULL */,
                            const uint8_t *open /* [n_utt]: 1 = tokens[u] is a head, text continues through text_cb */,
                            int32_t *codes, int32_t *n_frames, int32_t *held /* [n_utt] or NULL: times u was put on hold */,
                            int32_t max_active, q3t_queue_cb cb, void *user, int32_t interval,
                            q3t_text_cb text_cb, void *text_user);
/* counters of the context's last q3t_generate_queue_text with an open utterance (any pointer may be NULL): frame graphs
 * launched, loop rounds that launched none because every busy slot was held, feed rounds (one copy, the text projection
 * and the append / hold / release launches of one loop iteration) and their summed device time in ms */
int q3t_text_feed_stats(const q3t_ctx *ctx, int32_t *graph_launches, int32_t *idle_rounds, int32_t *feed_rounds,
                        double *feed_ms);
/* ---- the open queue: admit new utterances while continuous batching runs.  The utterances are not given up front:
 * `arrive` is asked for them on the caller's thread, between two frames, at most once per iteration of the frame loop and
 * only when no admission batch is in flight and room = min(free slots, max_active - busy slots) > 0.
 *   next_id  the id of the first utterance it returns (arrival order, from 0 per call; the rest follow)
 *   room     how many it may return: more is Q3T_ERR.  The engine keeps no backlog; a request that finds no room waits
 *            with the caller
 *   running  busy slots
 *   idle     1 exactly when no slot is busy: the callback may block until a request exists.  With idle == 0 it must
 *            return at once (the other utterances wait for it)
 * It fills out[0 .. *n) and sets *closed != 0 when no more will arrive after these; the call returns when the source is
 * closed and every accepted utterance has ended.  Return 0 to abort the call (Q3T_OK, as q3t_queue_cb).
 * Deliveries keep the contract of q3t_generate_queue_stream with utt[i] = the arrival id: increasing ids within a
 * callback, exactly one final delivery per utterance, a delivery that is neither an utterance's first nor its last has
 * exactly `interval` frames, stop[i] cancels.  Both callbacks get the same `user`.
 * An utterance that arrives with key k, record r, speaker s and tokens t gets, bit for bit and in length, the codes
 * q3t_generate_queue_utt returns for index k of a call at the same slots, seed and p->max_len in which utterance k has
 * (t, s, r): whenever it arrived, whatever else ran, whichever slot it took.
 * slots (<= 0: the context's max_slots) is fixed for the call; p gives max_len and seed.  Each arrival is validated with
 * the checks of q3t_generate_queue_utt (q3t_check_utt); an invalid one, or more than `room`, ends the call with Q3T_ERR
 * and a message naming its id, after both streams are drained.  Ids are int32: the call ends with Q3T_ERR when they run
 * out.  The host state is bounded by the slot count, not by the arrivals so far.
 * Lock rule: the call holds the context's device lock (devlock.h) from start to end, also while an idle ask blocks; at
 * slot counts that run persistent kernels that lock is exclusive, and other contexts on the device wait.
 * n_arrived / n_finished (may be NULL): utterances accepted / ended by a final delivery or a cancel. */
typedef struct q3t_arrival {
    const int32_t *tokens; int32_t n_tokens;   /* read before the callback returns */
    const float *speaker;                      /* hidden floats or NULL; read before the callback returns */
    q3t_utt_params up;
    uint64_t key;                              /* sampling key: (seed, key, frame, step) */
} q3t_arrival;
typedef int (*q3t_arrive_cb)(void *user, int32_t next_id, int32_t room, int32_t running, int32_t idle,
                             q3t_arrival *out, int32_t *n, int32_t *closed);
int q3t_generate_queue_open(q3t_ctx *ctx, const q3t_gen_params *p, int32_t slots, int32_t max_active,
                            q3t_arrive_cb arrive, q3t_queue_cb cb, void *user, int32_t interval, int32_t *n_arrived,
                            int32_t *n_finished);
/* what q3t_generate_queue_open (and q3t_generate_queue_utt) would refuse of one utterance: Q3T_ERR with the message in
 * q3t_last_error (it names utterance 0), Q3T_OK otherwise.  Nothing runs. */
int q3t_check_utt(const q3t_ctx *ctx, const int32_t *tokens, int32_t n_tokens, const float *speaker,
                  const q3t_gen_params *p, const q3t_utt_params *up);
/* tuning knob (process-wide): batches of >= min_batch slots run the projections on the matrix cores (MFMA GEMM,
 * gemm_mfma.hip) instead of the weight-streaming GEMV; 0 disables the matrix-core path.  Default 4 (env
 * Q3T_MFMA_MIN_B).  Applies to graphs captured afterwards (create contexts after changing it). */
int q3t_set_mfma_min_batch(int min_batch);
/* wait until every operation queued on the context's device has finished (hipDeviceSynchronize) */
int q3t_synchronize(q3t_ctx *ctx);
/* device time (ms) of the last q3t_generate: prefill and frame loop */
int q3t_last_timing(const q3t_ctx *ctx, double *prefill_ms, double *frames_ms);

/* replay the captured stage graph (0 = talker decode step, 1 = 16-pass code-predictor frame) `iters` times at
 * KV position `pos` for n_slots slots; *ms = mean device time per replay (an event pair around each replay on the
 * context stream: the replay's own duration, not the host-side gap between two graph launches) */
int q3t_time_stage(q3t_ctx *ctx, int stage, int n_slots, int pos, int iters, double *ms);
/* the single-slot talker step and code-predictor frame as persistent launches (persist.hip, no reference
 * counterpart: they replace the per-op graphs of TTSTransformer::forward_step / TRTCodePredictor at batch 1):
 * -1 = not in use (shapes or device not supported, another context on the device holds the persistent kernels, or
 * Q3T_PERSIST=0), 0 = in use, 1 = a launch gave up waiting on an in-launch hand-off (protocol fault; the next call
 * falls back), 2 = disabled after such a fault: the context runs the bit-identical launch-per-op graphs */
int q3t_persist_status(q3t_ctx *ctx);
/* which single-slot persistent kernels the context launches (bit mask, 0 when none): 1 = talker step on
 * role-specialised workgroups (persist_tk.hip), 2 = talker step on all-role workgroups (persist.hip k_persist<0,CH>),
 * 4 = code-predictor frame on role-specialised workgroups (persist_cp.hip), 8 = code-predictor frame on all-role
 * workgroups (persist.hip k_persist<1|2,16>) */
int q3t_persist_kernels(q3t_ctx *ctx);
/* which kernels a frame loop of n_slots slots launches on this context: 0 = the weight-streaming vector kernels (one
 * slot: as persistent launches where q3t_persist_kernels says so), 1 = the launch-per-op matrix-core stack (MFMA GEMMs,
 * hoisted norms, batched attention), 2 = the batched persistent launches (code-predictor frame and / or talker step).
 * Q3T_ERR for n_slots outside [1, max_slots].  A model with code_pred.mtp_proj (1.7B) reports 1 from 4 slots on, or 0 at
 * every slot count when the context was created under Q3T_MM17=0. */
int q3t_decode_family(q3t_ctx *ctx, int n_slots);

/* ---- vocoder */
int64_t q3t_vocoder_num_samples(const q3t_ctx *ctx, int32_t n_frames, int mode);
/* algorithmic FLOPs of one FULL decode of n_frames (sum of 2*M*K*N over the loaded conv / projection shapes and the
 * causal attention); bench.py's MFMA-utilisation figure.  -1 without a vocoder */
double q3t_vocoder_flops(const q3t_ctx *ctx, int32_t n_frames);
int q3t_vocoder_decode(q3t_ctx *ctx, const int32_t *codes /* [n_frames][16] */, int32_t n_frames, int mode,
                       float *pcm /* [q3t_vocoder_num_samples] */, int64_t *n_samples);

/* TRTVocoderDecoder::decode (src/trt_vocoder.h:33-34) with the engine's fixed_frames: independent chunk_frames-long
 * chunks, n_frames * 1920 samples (pcm capacity); n_codebooks must be 16 */
int q3t_vocoder_decode_chunked(q3t_ctx *ctx, const int32_t *codes /* [n_frames][n_codebooks] */, int32_t n_frames,
                               int32_t n_codebooks, int32_t chunk_frames, float *pcm, int64_t *n_samples);

/* Several utterances through shared launches (the batched counterpart of q3t_vocoder_decode /
 * q3t_vocoder_decode_chunked; the reference decodes one utterance per call, qwen3_tts.cpp:518 /
 * trt_vocoder.cpp:98-170).  FULL: utterances run as batches of up to q3t_vocoder_set_batch_frames frames (default
 * 4096), each padded to its batch's longest; the decoder is causal end to end, so pcm[u] is exactly
 * q3t_vocoder_decode(codes[u]).  CHUNK40: every chunk_frames-long chunk of every utterance is one independent sequence
 * of the batch; pcm[u] equals q3t_vocoder_decode_chunked(codes[u]).  codes[u]: [n_frames[u]][16];
 * pcm[u]: capacity q3t_vocoder_num_samples(n_frames[u], mode); n_samples[u] receives its length. */
int q3t_vocoder_decode_batch(q3t_ctx *ctx, int32_t n_utt, const int32_t *const *codes, const int32_t *n_frames,
                             int mode, int32_t chunk_frames, float *const *pcm, int64_t *n_samples);
/* frames (utterances x frames) per batched vocoder launch sequence; scratch grows to ~3 MB per frame */
int q3t_vocoder_set_batch_frames(q3t_ctx *ctx, int32_t frames);

/* Streaming FULL decode: frames pushed in pieces of any size; the concatenation of the PCM of the pushes is, bit for
 * bit, q3t_vocoder_decode(all frames, Q3T_VOCODER_FULL).  After F frames in total the stream has emitted exactly
 * q3t_vocoder_num_samples(F, Q3T_VOCODER_FULL) samples, and a push returns the difference from the previous total
 * (there is no flush: the one-shot decode of the same frames ends at the same sample).  The frame-rate part runs on
 * the new frames only, against state the stream carries (per-layer f32 K/V caches sized at open from max_frames,
 * ~64 KB per frame with the shipped geometry; open fails when they do not fit); the convolution stack is recomputed
 * over the last q3t_vocoder_stream_halo frames plus the new ones.  The cost of a push depends on the piece, not on
 * the history, except for the attention over the cached keys.
 * Several streams may be open on one context, each with its own state; pushes, q3t_vocoder_decode and
 * q3t_vocoder_decode_batch on the same context may interleave freely (they share the decoder's scratch and run one
 * after the other on the context stream, under the device lock q3t_vocoder_decode takes).  A push may be made from a
 * q3t_generate_stream callback, under the rule stated there for q3t_vocoder_decode.
 * Q3T_ERR with a message, the stream's state unchanged: n_frames <= 0, more than max_frames frames in total, pcm_cap
 * smaller than the push's sample count, a context without a vocoder (open).  A push writes
 * q3t_vocoder_num_samples(frames + n_frames, Q3T_VOCODER_FULL) - q3t_vocoder_stream_samples samples.
 * q3t_ctx_destroy frees the streams still open on the context; their handles are invalid afterwards.
 * Q3T_VOC_STREAM_HALO=<frames> (development knob, read at open) overrides the derived halo. */
typedef struct q3t_voc_stream q3t_voc_stream;
int q3t_vocoder_stream_open(q3t_ctx *ctx, int32_t max_frames, q3t_voc_stream **out);
int q3t_vocoder_stream_push(q3t_voc_stream *s, const int32_t *codes /* [n_frames][16] */, int32_t n_frames,
                            float *pcm, int64_t pcm_cap, int64_t *n_samples);
int64_t q3t_vocoder_stream_samples(const q3t_voc_stream *s); /* emitted so far */
int32_t q3t_vocoder_stream_frames(const q3t_voc_stream *s);  /* pushed so far */
int32_t q3t_vocoder_stream_halo(const q3t_voc_stream *s);    /* frames of left context the convolution stack re-runs */
void q3t_vocoder_stream_close(q3t_voc_stream *s);
/* rewind an open stream to zero frames and zero samples, keeping its caches (and the carried tails and halos, which a
 * push reads only as far as the frame count reaches): the pushes after a reset give, bit for bit, the PCM of a fresh
 * stream.  A serving loop keeps one stream per slot instead of opening and closing one per utterance (which allocates
 * and frees the per-layer K/V caches and synchronises the device).  Q3T_ERR: a null or closed stream. */
int q3t_vocoder_stream_reset(q3t_voc_stream *s);

/* One push on each of n_streams streams through shared launches, for batched serving.  All streams belong to one
 * context; they may stand at any positions and take any mix of n_frames.  codes[j]: [n_frames[j]][16]; pcm[j]: capacity
 * pcm_cap[j] samples; n_samples[j] receives stream j's count.  Stream j's PCM is bit-identical to pushing it alone with
 * q3t_vocoder_stream_push, so the concatenation over its pushes, batched or single in any mix, is still
 * q3t_vocoder_decode(all frames, Q3T_VOCODER_FULL).  The frame-rate part runs once over the new frames of all streams
 * (the attention and the cache append serve every stream's cache in one launch each per layer); the convolution
 * stack runs once per group of streams with equal n_frames and equal carried history (min(frames, halo)), so streams
 * in the steady state that push the same number of frames share every launch.  q3t_vocoder_stream_last_groups
 * returns the number of such groups (convolution-stack launch sequences) of the context's last batched push, -1 on a
 * null context.  The call takes the device lock a push takes and synchronises once.
 * Q3T_ERR with a message, EVERY stream's state unchanged and every n_samples[j] = 0: n_streams <= 0, a null array or
 * entry, a stream that is not open on the first stream's context, a stream given twice, and for any stream
 * n_frames <= 0, more than max_frames frames in total, or pcm_cap smaller than the push's sample count. */
int q3t_vocoder_stream_push_batch(q3t_voc_stream *const *streams, int32_t n_streams,
                                  const int32_t *const *codes, const int32_t *n_frames,
                                  float *const *pcm, const int64_t *pcm_cap, int64_t *n_samples);
int32_t q3t_vocoder_stream_last_groups(const q3t_ctx *ctx);

/* ---- output stage: resampled f32 / s16 / mu-law PCM from decodes and streams, converted on the device so that only
 * the client's bytes are copied back.  The input is the vocoder's f32 at its native rate (24000).  Rates: 8000, 12000,
 * 16000, 22050, 24000, 32000, 44100, 48000; anything else is Q3T_ERR with a message naming the rate and the list.  The
 * resampler is a causal polyphase FIR (Kaiser-windowed sinc, 16 zero crossings a side, cut-off 0.9 of the lower
 * Nyquist; DESIGN 2c "Output stage" states it exactly) whose every output sample is one fmaf chain in a fixed order:
 * a stream's bytes do not depend on how its frames were cut into pushes or on which streams shared a launch, and the
 * concatenation over its pushes (the last one final) is, byte for byte, q3t_vocoder_decode_out of all frames.
 * After S input samples a stream has produced ceil(S * L / M) outputs (L / M = rate / 24000 in lowest terms); the
 * filter delays the signal by 16 * max(L, M) / L input samples (0.67 .. 2 ms, not compensated); a final push appends
 * D = ceil(16 * max(L, M) / L) zero samples once, so the tail is emitted.  24000 bypasses the filter: the output is
 * the input bit for bit, and final adds nothing.
 * s16: (int16)(clamp(y, -1, 1) * 32767.0f), truncated toward zero (the WAV writer's rule); mu-law: G.711 of that. */
#define Q3T_PCM_F32 0
#define Q3T_PCM_S16 1
#define Q3T_PCM_MULAW 2
typedef struct q3t_pcm_spec { int32_t sample_rate; int32_t format; } q3t_pcm_spec;
/* host-only helpers (no device touched) */
int32_t q3t_pcm_bytes_per_sample(int32_t format);   /* 4 / 2 / 1; 0 for an unknown format */
/* outputs after n_in_total input samples (final != 0: with the tail); -1 for an unsupported rate */
int64_t q3t_pcm_num_samples(int64_t n_in_total, int32_t sample_rate, int32_t final);
/* the exact f32 tap table the kernel uses, [L][K] row-major, taps[p][k] = (float)(L * h[p + k * L]); taps == NULL
 * queries L, M, K.  24000 has K = 0 (no table).  Q3T_ERR: an unsupported rate, cap < L * K */
int q3t_pcm_taps(int32_t sample_rate, int32_t *L, int32_t *M, int32_t *K, float *taps, int64_t cap);
/* one-shot decode (FULL or CHUNK40) through the stage with final = 1: *n_samples samples of spec->format into out
 * (q3t_pcm_num_samples(q3t_vocoder_num_samples(n_frames, mode), rate, 1) of them) */
int q3t_vocoder_decode_out(q3t_ctx *ctx, const int32_t *codes /* [n_frames][16] */, int32_t n_frames, int mode,
                           const q3t_pcm_spec *spec, void *out, int64_t out_cap_bytes, int64_t *n_samples);
/* give a stream an output spec: only at zero frames (fresh or reset), Q3T_ERR otherwise; spec == NULL clears it.
 * q3t_vocoder_stream_reset keeps the spec and rewinds the stage (history zeroed, counts 0).  A stream with a spec is
 * pushed with the _out calls only (the plain pushes return Q3T_ERR, state unchanged) and a stream without one with the
 * plain calls only; a stream that never had a spec behaves exactly as before. */
int q3t_vocoder_stream_set_output(q3t_voc_stream *s, const q3t_pcm_spec *spec);
/* q3t_vocoder_stream_push through the stage: *n_samples samples of the stream's format into out.  final != 0 emits
 * the tail; after it the stream takes no further output push until it is reset.  An extension over the plain push: a
 * final push may carry no frames (n_frames == 0, codes ignored) and then only flushes the tail, for an utterance whose
 * last queue delivery is empty.  Errors as q3t_vocoder_stream_push (out_cap_bytes in place of pcm_cap; n_frames == 0
 * without final), state unchanged.  A device error after the frames were taken leaves the stream refusing output pushes
 * until q3t_vocoder_stream_reset (its samples for the stage are gone). */
int q3t_vocoder_stream_push_out(q3t_voc_stream *s, const int32_t *codes /* [n_frames][16] */, int32_t n_frames,
                                int32_t final, void *out, int64_t out_cap_bytes, int64_t *n_samples);
/* q3t_vocoder_stream_push_batch through the stage.  Streams of one call may carry different specs; each stream's bytes
 * are those of pushing it alone.  The call adds ONE conversion launch (plus the history update) to the launches of
 * q3t_vocoder_stream_push_batch, and its device-to-host copies carry output bytes only.  final: [n_streams] or NULL
 * (none).  Error contract of q3t_vocoder_stream_push_batch: every stream unchanged, every n_samples[j] = 0. */
int q3t_vocoder_stream_push_batch_out(q3t_voc_stream *const *streams, int32_t n_streams, const int32_t *const *codes,
                                      const int32_t *n_frames, const int32_t *final /* [n_streams] or NULL */,
                                      void *const *out, const int64_t *out_cap_bytes, int64_t *n_samples);
int64_t q3t_vocoder_stream_out_samples(const q3t_voc_stream *s); /* output samples so far; -1 without a spec */
/* diagnostic, not part of the serving interface: k_pcm_out launches made by this process so far (a successful call of
 * the _out pushes or of q3t_vocoder_decode_out adds exactly one); process-wide, for tests and tools/dev/pcm_out_bench.py */
int64_t q3t_pcm_out_launches(void);

/* ---- speaker encoder (ECAPA-TDNN; the TTS GGUF's spk_enc.* tensors)
 * q3t_speaker_dim: embedding length, 0 when the model has no speaker encoder.
 * q3t_speaker_encode: AudioTokenizerEncoder::encode (src/audio_tokenizer_encoder.h:107-108): samples in [-1, 1] at
 * 24 kHz -> embedding [q3t_speaker_dim]; Q3T_ERR + q3t_last_error() when the audio is too short (< 5 mel frames).
 * q3t_speaker_mel: its log-mel front end (compute_mel_spectrogram, audio_tokenizer_encoder.cpp:281-364), time-major
 * [n_frames][128]; mel may be NULL to query *n_frames. */
int q3t_speaker_dim(const q3t_ctx *ctx);
/* a context holding only the speaker encoder (AudioTokenizerEncoder::load_model reads only spk_enc.* tensors) */
int q3t_ctx_create_speaker(const char *tts_gguf, int device, q3t_ctx **out);
int q3t_speaker_encode(q3t_ctx *ctx, const float *samples, int32_t n_samples, float *embedding);
/* q3t_speaker_encode_batch: n_clips clips of any lengths through shared launches (one host-to-device copy and one
 * launch train per group instead of one per clip).
 * Contract: embeddings[c] equals, bit for bit, what q3t_speaker_encode gives for samples[c] alone -- whatever the other
 * clips, its position in the batch or the batch size.
 * Groups: clips are packed in order, 8 rows apart, into groups of at most Q3T_SPK_GROUP_ROWS packed rows (mel frames + 8
 * per clip; default 4096, about 43 s of audio; the environment variable is read at each call).  The bound keeps every
 * conv of a group on the kernel instance a clip alone gets; the call checks that on the host for every group and
 * encodes a group clip by clip if it does not hold.  A clip longer than a group is encoded alone.
 * Errors: a clip with fewer than 5 mel frames (or fewer than 2 samples, or a NULL pointer) gets ok[c] = 0 and a zeroed
 * row, takes no device work and does not fail the others (ok[c] = 1).  With ok == NULL such a clip fails the whole
 * call before any device work; q3t_last_error() names its index.  n_clips == 0 is Q3T_OK.
 * Takes the device lock as q3t_speaker_encode does, so it may be called from a queue callback on the caller's thread,
 * and works on a q3t_ctx_create_speaker context.
 * q3t_speaker_launches: kernel launches of the speaker encoder so far, process-wide (a conv counts 2: its pad launch
 * and its conv launch); for tests and tools/dev/speaker_batch_bench.py. */
int q3t_speaker_encode_batch(q3t_ctx *ctx, const float *const *samples, const int32_t *n_samples, int32_t n_clips,
                             float *embeddings /* [n_clips][q3t_speaker_dim] */, int32_t *ok /* [n_clips] or NULL */);
int64_t q3t_speaker_launches(void);
int q3t_speaker_mel(q3t_ctx *ctx, const float *samples, int32_t n_samples, float *mel, int32_t cap_frames,
                    int32_t *n_frames);

/* ---- text tokenizer (host side; TextTokenizer, src/text_tokenizer.h:21-86 / text_tokenizer.cpp:80-349)
 * q3t_tokenizer_load reads tokenizer.ggml.tokens / merges / *_token_id from a GGUF (the TTS model file).
 * q3t_tokenizer_encode: for_tts != 0 wraps the text in the TTS template (encode_for_tts, :293-330); *n_tokens receives
 * the count, tokens may be NULL to query it, Q3T_ERR when cap is too small.
 * q3t_tokenizer_decode: bytes of the decoded text (not NUL-terminated), *n_bytes its length; text may be NULL. */
typedef struct q3t_tokenizer q3t_tokenizer;
int q3t_tokenizer_load(const char *gguf_path, q3t_tokenizer **out);
void q3t_tokenizer_free(q3t_tokenizer *tok);
int q3t_tokenizer_info(const q3t_tokenizer *tok, int32_t *vocab_size, int32_t *bos_id, int32_t *eos_id,
                       int32_t *pad_id);
int q3t_tokenizer_encode(const q3t_tokenizer *tok, const char *text, int64_t n_bytes /* < 0: NUL-terminated */,
                         int for_tts, int32_t *tokens, int32_t cap, int32_t *n_tokens);
int q3t_tokenizer_decode(const q3t_tokenizer *tok, const int32_t *tokens, int32_t n, char *text, int64_t cap,
                         int64_t *n_bytes);

/* ---- stage entry points (used by the parity tests; each syncs the context stream) */
int q3t_talker_forward(q3t_ctx *ctx, int n_slots, const float *embd /* [n][H] */, const int32_t *pos /* [n] */,
                       float *hidden /* [n][H] or NULL */, float *logits /* [n][codec_vocab] or NULL */);
/* causal prefill from position 0 (the pass q3t_generate runs): the n_rows <= 10 rows of each of n_utt utterances in one
 * pass, K/V into slots 0..n_utt-1; hidden = the final-norm hidden state of every row, logits = the codec logits of each
 * utterance's last row.  family_slots (0: n_utt) picks the kernels of a family_slots-slot decode step: every row then
 * equals q3t_talker_forward with that many slots replayed at its position, bit for bit. */
int q3t_talker_prefill(q3t_ctx *ctx, int n_utt, int n_rows, const float *embd /* [n_utt][n_rows][H] */, int family_slots,
                       float *hidden /* [n_utt][n_rows][H] or NULL */, float *logits /* [n_utt][codec_vocab] or NULL */);
/* the same over prompts of different lengths in one pass: utterance u has n_rows[u] (1..10) rows, packed one utterance
 * after the other in embd and hidden; logits [n_utt][codec_vocab].  Row i of utterance u is, bit for bit, what
 * q3t_talker_prefill(n_utt = 1, n_rows = n_rows[u]) computes for it (hidden, last-row logits, the K/V rows of slot u). */
int q3t_talker_prefill_ragged(q3t_ctx *ctx, int n_utt, const int32_t *n_rows /* [n_utt] */, const float *embd,
                              int family_slots, float *hidden /* packed, or NULL */, float *logits /* or NULL */);
int q3t_codepred_frame(q3t_ctx *ctx, int n_slots, const float *hidden /* [n][H] */, const int32_t *cb0 /* [n] */,
                       float temperature, int32_t top_k, uint64_t seed, int32_t frame,
                       int32_t *codes15 /* [n][15] */, float *logits /* [n][15][cp_vocab] or NULL */);
int q3t_cb0_select(q3t_ctx *ctx, int n_slots, const float *logits /* [n][V] */, const uint8_t *seen /* [n][V] */,
                   const int32_t *frame, const int32_t *n_tokens, const q3t_gen_params *p, int32_t *tokens);
int q3t_project_text(q3t_ctx *ctx, int n, const int32_t *tokens, float *out /* [n][H] */);
int q3t_prefill_embd(q3t_ctx *ctx, const int32_t *tokens, int n, const float *speaker, int language_id,
                     float *prefill /* [10][H] */, int32_t *prefill_len, float *trailing /* [max(1,n-8)][H] */,
                     int32_t *trailing_len, float *tts_pad /* [H] */);

/* ---- drop-in replacements of src/trt_cuda_kernels.cu (device pointers, stream = hipStream_t or NULL) */
void gpu_fp32_to_fp16(const float *in, void *out, int n, void *stream);
void gpu_argmax_f32(const float *in, int32_t *out, int n, void *stream);
void gpu_embedding_lookup_by_gpu_id(const int32_t *token_id_ptr, const float *table, float *output, int embd_dim,
                                    void *stream);
void gpu_sample_topk_f32(const float *logits, const float *rand_val, int32_t *out, float temperature, int32_t top_k,
                         int32_t vocab_size, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* Q3T_BACKEND_H */
