// engine.h — MI355X-native runtime of the per-frame decode path (Talker step -> CB0 -> Code Predictor ->
// step embedding), replacing the reference's TTSTransformer::generate hot loop (src/tts_transformer.cpp:2342-2574)
// and TRTCodePredictor (src/trt_code_predictor.cpp).  B utterances ("slots") advance in lock-step; every
// per-frame kernel reads positions / frame counters from device memory so one hipGraph replays every frame.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "arena.h"
#include "gguf.h"
#include "kernels.h"
#include "queue_deliver.h"
#include "queue_sched.h"

namespace q3t {

struct Config {
    int hidden = 1024, n_layers = 28, n_heads = 16, n_kv = 8, head_dim = 128, inter = 3072;
    int codec_vocab = 3072, n_codebooks = 16, text_vocab = 151936, text_dim = 2048;
    int cp_layers = 5, cp_vocab = 2048;
    // code predictor geometry (tts_transformer.cpp:370-389): the talker's values for 0.6B; 1.7B has its own hidden /
    // FFN width behind code_pred.mtp_proj (talker space -> code-predictor space, applied to every pass input)
    int cp_hidden = 1024, cp_inter = 3072, cp_heads = 16, cp_kv = 8;
    bool has_mtp = false;
    float eps = 1e-6f, rope_theta = 1e6f;
    int codec_pad = 2148, codec_bos = 2149, codec_eos = 2150;
    int tts_bos = 151672, tts_eos = 151673, tts_pad = 151671;
    int think = 2154, nothink = 2155, think_bos = 2156, think_eos = 2157;
};

struct GenParams {
    int max_len = 4096;
    int language_id = 2050;
    float rep_penalty = 1.05f;
    float temperature = 0.9f;
    int top_k = 50;
    uint64_t seed = 0;
    int force_frames = 0;      // bench: mask EOS until this many frames are produced
};

// (UttParams, one utterance's own values, is queue_sched.h's: the arrival log keeps a copy per utterance)

struct DevLayer {
    uint16_t *qkv = nullptr, *o = nullptr, *gu = nullptr, *down = nullptr;
    float *attn_norm = nullptr, *ffn_norm = nullptr, *qn = nullptr, *kn = nullptr;
};

class Vocoder;
class SpeakerEncoder;
struct PLayerW;

// scratch of one prompt assembly in flight (Engine::assemble_prompts): one set per stream that assembles prompts
struct PromptScratch {
    int cap = 0;                   // rows of idx / h / out / recipe
    int *idx = nullptr;            // text token id per projection row
    uint16_t *h = nullptr;         // fc1 output (f16)
    float *out = nullptr;          // projected text rows
    RowRecipe *recipe = nullptr;
    float *rows = nullptr;         // prompt rows [max_slots][10][H] (ragged assemblies pack them: PromptEntry::row)
    float *spk = nullptr;          // speaker rows [max_slots][H], by target slot
    std::vector<int> idx_host;     // the (pageable) sources of the idx / recipe uploads: they outlive the copies
    std::vector<RowRecipe> recipe_host;
    std::vector<int> rag_host;     // ragged prefill: [n] row offsets, then [n] row counts
    std::vector<SelRec> rec_host;  // per-utterance sampling: the slots' records of a lock-step call
};
// one utterance of an assembly: its speaker row (or null), the slot whose trailing / pad rows it fills, the first
// row of its prompt in PromptScratch::rows (10 x its index in the uniform layout, the running sum of the lengths in
// the packed one) and its language
struct PromptEntry {
    const int32_t *tokens;
    int n_tokens;
    const float *speaker;
    int slot, row;
    int language_id;
};

// Path-selection knobs, read once from the environment when a context is created (the reference's own pattern:
// QWEN3_TTS_LOW_MEM, src/qwen3_tts.cpp:125-129).  All default to the fastest path; the alternatives exist so that
// the tests can compare paths that must agree (persistent vs launch-per-op, sequential vs split attention).
//   Q3T_PERSIST=0          single-slot talker step as launch-per-phase graphs instead of the persistent kernel
//   Q3T_PERSIST_CP=0       single-slot code-predictor frame as per-op launches
//   Q3T_PERSIST_CPB=0      batched (matrix-core) code-predictor frame as per-op launches (persist_cpb.hip otherwise)
//   Q3T_PERSIST_TKB=0      batched (matrix-core) talker step as per-op launches (persist_tkb.hip otherwise)
//   Q3T_CP_FUSED_ATTN=0    code-predictor attention as its own launch (the arithmetic the persistent frame reproduces)
//   Q3T_FUSED_SELECT=0     token selection as standalone launches
//   Q3T_CP_DEFER_SELECT=0  code-predictor tokens selected in the head launch
//   Q3T_ATTN_SPLIT=1       batched attention always split-K (k_attn) instead of k_attn_seq at >= 16 slots
//   Q3T_MM_PREFETCH=1|2    batched talker stack: weight prefetch from the norms (1) and also the gate/up GEMM (2)
//   Q3T_MM_GU_TT=1         batched stacks: gate/up GEMM on 32-token tiles instead of 64
//   Q3T_PERSIST_FAULT_AT=n test hook: the n-th persistent launch of the context flags a hand-off fault
// Development-only knobs (Q3T_TALKER_LAYERS, Q3T_PERSIST_PROF, ...) exist only in a -DQ3T_DEV build.
struct Options {
    bool persist = true, persist_cp = true, cp_fused_attn = true, fused_select = true, defer_cp_select = true;
    bool cp_qkv_table = true;   // Q3T_CP_QKV_TABLE: the persistent code-predictor frame reads layer 0's QKV rows from a table
    bool cp_roles = true;       // Q3T_CP_ROLES: that frame on role-specialised workgroups (persist_cp.hip)
    bool mm_cp_table = true;    // Q3T_MM_CP_TABLE: batched code predictor, layer 0 of passes 1..15 from the QKV table
    bool fold_advance = true;   // Q3T_FOLD_ADVANCE: the single-slot role talker kernel advances pos / frame (no k_advance)
    bool tk_roles = true;       // Q3T_TK_ROLES: the 1-slot talker step on role-specialised workgroups (persist_tk.hip)
    bool cpb = true;            // Q3T_PERSIST_CPB: the batched (2..64-slot) code-predictor frame as one persistent launch
    bool tkb = true;            // Q3T_PERSIST_TKB: the batched (16..64-policy-slot) talker step as one persistent launch
    bool attn_split = false;
    bool mm17 = true;           // Q3T_MM17: models with code_pred.mtp_proj (1.7B) on the batched matrix-core stack
    int mm_prefetch = 0;        // Q3T_MM_PREFETCH (from_env)
    int mm_gu_tt = 2;           // Q3T_MM_GU_TT: gate/up token tile in 32-token units (from_env)
    unsigned persist_fault_at = 0;
    int poll_every = 16;   // frames between done-flag polls
    static Options from_env();
};

// what one run of a launch-per-op decoder stack (engine.cpp: decoder_stack / decoder_stack_mm) computes in, and the
// cache it attends over
struct StackBufs {
    float *x, *parts, *qkv;       // residual stream, split-K partial slabs (matrix-core path), raw QKV rows
    uint16_t *xn, *attn, *hmlp;   // normalised rows (matrix-core path), attention output, SwiGLU output
};
struct StackCache {
    uint16_t *kc, *vc;
    size_t kv_layer;              // elements of one layer's cache
    int n_ctx, max_splits;
    const int *pos;               // [S] position of each slot's new token
    const float *rope;
    float *part; unsigned *ticket;   // split attention: partials and arrival counters
};

class Engine {
public:
    Engine();
    ~Engine();
    // recv_weights: lay out the weight arenas from the GGUF headers only; the bytes are filled afterwards by
    // copy_weights_from() or an RCCL broadcast of weight_arenas()
    // host-only weight layout of a model file (no device): allocation offsets in order, bytes used
    bool plan_layout(const std::string &tts_gguf, std::vector<size_t> &offsets, size_t &used);
    bool load(const std::string &tts_gguf, const std::string &tok_gguf, int device, int max_slots, int max_ctx,
              bool recv_weights = false);
    // the packed weight blobs (talker + code predictor + embeddings; vocoder), in broadcast order
    std::vector<WeightArena *> weight_arenas();
    const Config &cfg() const { return c_; }
    int max_slots() const { return max_slots_; }
    int device() const { return device_; }
    const std::string &tts_path() const { return tts_path_; }
    // speaker-encoder-only context (AudioTokenizerEncoder::load_model, audio_tokenizer_encoder.cpp: only the
    // spk_enc.* tensors of the TTS GGUF are read)
    bool load_speaker_only(const std::string &tts_gguf, int device);
    bool has_talker() const { return talker_; }
    const std::string &tok_path() const { return tok_path_; }
    int max_ctx() const { return max_ctx_; }
    hipStream_t stream() const { return stream_; }
    Vocoder *vocoder() { return voc_.get(); }
    SpeakerEncoder *speaker() { return spk_.get(); }   // null when the TTS GGUF has no spk_enc.* tensors

    // ---- hot path: prefill + frame loop for n_utt utterances (codes [n_utt][max_len][ncb])
    // on_frames (frame_callback_t, src/tts_transformer.h:224): called every `interval` frames per utterance with its
    // newest `interval` frames, plus one final flush of the remainder; returning 0 stops that utterance
    // (src/tts_transformer.cpp:2517-2523, 2563-2570)
    typedef int (*FrameCb)(void *user, int slot, const int32_t *codes, int n_frames, int n_codebooks);
    // up (q3t_generate_utt / q3t_generate_queue_utt): [n_utt] records; gp then gives only max_len (the stride of codes and
    // the cap of every record) and the seed, and speaker[u] may be null for any subset.  Null: the call-wide gp.
    bool generate(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                  const GenParams &gp, int32_t *codes, int *n_frames, FrameCb on_frames = nullptr,
                  void *user = nullptr, int interval = 40, const UttParams *up = nullptr);
    // continuous batching: n_utt utterances (any number) through min(max_slots, n_utt) slots, at
    // most max_active of them at a time.  A slot whose utterance ended (EOS or max_len) is refilled with the next
    // queued utterance between two frames.  The slots freed since the last admission are admitted together, on the
    // admission stream while the other slots go on decoding: their text rows are projected, their prompt rows assembled
    // and run through one causal prefill that writes K/V straight into the target slots; each slot then joins the
    // frame loop on the main stream with its state (position, frame, EOS, repetition set, codes) reset.  Sampling
    // streams are keyed by the utterance's index in the call (utt id), so an utterance's codes do not depend on its
    // slot, its admission frame or the other utterances in flight (the S-slot decode step never mixes tokens); the
    // admission prefill runs the running batch's kernels, whose per-row arithmetic does not depend on the other rows,
    // so the first wave's codes equal generate()'s.
    // on_batch (q3t_queue_cb) with interval > 0: the queue hands frames out while it runs (DESIGN 2f "Queue
    // deliveries").  Every `interval` frames of the loop clock one collection launch gathers the new frames of all
    // active slots (a tick); when a slot's utterance ends, one more gathers the rest of the finished slots and is
    // marked final.  One callback per collection: n entries in increasing utterance index, codes[i] -> [n_frames[i]][16]
    // valid during the call, final[i] on the utterance's last delivery; stop[i] set non-zero cancels utterance utt[i]
    // (its slot is parked, freed and refilled; n_frames[u] = the frames delivered); returning 0 aborts the call
    // (n_frames = the frames delivered).  With a callback codes may be null: no per-utterance device copy is kept.
    typedef int (*QueueCb)(void *user, int32_t n, const int32_t *utt, const int32_t *const *codes, const int32_t *n_frames,
                           const int32_t *final, int32_t *stop);
    // text (q3t_generate_queue_text; DESIGN 2f "Text feeds"): utterances with open[u] != 0 are given as a head (three
    // role ids and >= 1 text id, no five-id suffix) and their further text ids come from cb, asked on the caller's thread
    // between two frames; a slot that has consumed every row it knows is held until more text (or its end) arrives.
    // interval > 0 is then required with or without on_batch (the clock of the asks).  held[u] (may be null): how often
    // utterance u was put on hold.
    typedef int (*TextCb)(void *user, int32_t utt, int32_t frames, int32_t rows_ahead, const int32_t **ids, int32_t *n_ids,
                          int32_t *end);
    struct TextFeed {
        const uint8_t *open = nullptr;   // [n_utt]
        TextCb cb = nullptr;
        void *user = nullptr;
        int32_t *held = nullptr;         // [n_utt]
    };
    bool generate_queue(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                        const GenParams &gp, int32_t *codes, int *n_frames, int max_active, QueueCb on_batch = nullptr,
                        void *user = nullptr, int interval = 0, const UttParams *up = nullptr, const TextFeed *text = nullptr);
    // the open queue (q3t_generate_queue_open; DESIGN 2f "Arrivals"): the utterances come from `arrive`, asked on the
    // caller's thread between two frames under the rules of queue_sched.h's ArrivalPlanner, and leave through on_batch
    // (required, interval > 0) under the delivery contract above with utt[i] = the arrival id.  slots (<= 0: max_slots) is
    // fixed for the call: it chooses the kernel family.  Every utterance runs with its own record (the records path) and
    // the ragged prefill, its sampling keyed by its arrival's key: its codes are those of index `key` of a closed call
    // with records at the same slots, seed and gp.max_len.  The device lock is held for the whole call, also while an
    // idle ask blocks.  gp gives max_len and the seed.
    typedef ArrivalPlanner::AskFn ArriveCb;
    bool generate_queue_open(const GenParams &gp, int slots, int max_active, ArriveCb arrive, QueueCb on_batch, void *user,
                             int interval, int32_t *n_arrived, int32_t *n_finished);
    // what the open queue would refuse of one utterance (q3t_check_utt): the message, or empty.  id: the utterance the
    // message names; *up: the record with max_len resolved, *plen: its prompt rows
    std::string check_arrival(int32_t id, const Arrival &a, const GenParams &gp, UttParams *up, int *plen);
    // counters of the last generate_queue with text feeds (q3t_text_feed_stats): frame graphs launched, loop rounds that
    // launched none because every busy slot was held, feed rounds (one copy + projection + k_text_append / hold /
    // release launches each) and the device time of those rounds (an event pair around each)
    struct TextStats { int graph_launches = 0, idle_rounds = 0, feed_rounds = 0; double feed_ms = 0; };
    TextStats text_stats;
    // fill this context's weight arenas (laid out with recv_weights) from another context's, device to device
    bool copy_weights_from(Engine &src);
    // after the weight arenas of a receiving context were filled by a broadcast: build what is derived from the weights
    // (the persistent code-predictor frame's per-token tables)
    bool finish_weights();

    // ---- stage entry points (host buffers) used by the parity tests
    bool talker_prefill(int n_utt, int n_rows, const float *embd, int family_slots, float *hidden, float *logits);
    // n_rows[u] in [1, 10] packed rows per utterance: the ragged form of the prefill (hidden packed, logits [n_utt][V])
    bool talker_prefill_ragged(int n_utt, const int *n_rows, const float *embd, int family_slots, float *hidden, float *logits);
    bool talker_forward(int S, const float *embd, const int *pos, float *hidden, float *logits);
    bool codepred_frame(int S, const float *hidden, const int *cb0, float temperature, int top_k, uint64_t seed,
                        int frame, int32_t *codes15, float *logits_all);
    bool cb0_select_host(int S, const float *logits, const uint8_t *seen, const int *frame, const int *n_tokens,
                         const GenParams &gp, int *tokens);
    bool project_text(int n, const int32_t *toks, float *out);
    bool prefill_embd(const int32_t *toks, int n, const float *spk, int language_id, float *prefill, int *prefill_len,
                      float *trailing, int *trailing_len, float *tts_pad);

    // replay the captured talker-step (or code-predictor frame) graph `iters` times at position `pos` for S slots and
    // report the mean device time per replay (HIP events on the context stream)
    bool time_stage(int stage, int S, int pos, int iters, double *ms);

    // true if a persistent launch gave up waiting on a hand-off (never expected: a protocol fault)
    bool persist_fault_hook(int S, int n_launches);   // Q3T_PERSIST_FAULT_AT test hook (host side)
    unsigned persist_launches_ = 0;
    bool persist_error();
    bool persist_enabled() const { return persist_ || persist_cp_ || cpb_ || tkb_; }
    int persist_kernels() const {   // q3t_persist_kernels
        return (persist_ ? (tk_roles_ ? 1 : 2) : 0) | (persist_cp_ ? (cp_roles_ && cp_qkvtab_ ? 4 : 8) : 0) | (cpb_ ? 16 : 0) | (tkb_ ? 32 : 0);
    }
    // q3t_decode_family: what a frame loop of S slots launches -- 0 the weight-streaming vector kernels (and the one-slot
    // persistent kernels built on them), 1 the launch-per-op matrix-core stack, 2 the batched persistent launches
    int decode_family(int S) const {
        if (S < 1 || S > max_slots_) return -1;
        return use_cpb(S) || use_tkb(S) ? 2 : use_mm(S) ? 1 : 0;
    }
    // runs with S slots launch a persistent grid (the 1-slot kernels, or the batched code-predictor frame / talker
    // step): they hold the device lock exclusively (devlock.h)
    bool persist_exclusive(int S) const { return ((persist_ || persist_cp_) && S == 1) || ((cpb_ || tkb_) && S > 1); }
    bool persist_fell_back() const { return persist_fallback_; }
#ifdef Q3T_DEV
    // development hook: copy a device state buffer to the host (0 K cache, 1 V cache, 2 qkv, 3 attention output)
    bool debug_read(int which, void *dst, size_t bytes);
#endif

    // profiling hooks for bench.py: last generate() timings
    double last_prefill_ms = 0, last_frames_ms = 0;

private:
    bool upload_weights(const Gguf &g);
    bool parse_config(const Gguf &g);
    bool layout_weights(const Gguf &g);
    bool upload_weights_rest();
    bool alloc_state();
    bool setup_persist(int n_cu);
    bool upload_layer_table(const std::vector<DevLayer> &layers, PLayerW *&dev);
    bool upload_head_table();
    // after a persistent launch flagged a fault: drain the stream, clear the hand-off state, drop the captured graphs
    // and continue on the launch-per-op graphs (the reference's permanent-fallback pattern, tts_transformer.cpp:2176-2182)
    bool persist_recover();
    struct StreamState {   // per utterance, kept across a fallback re-run so no chunk is delivered twice
        std::vector<int> delivered, stop_at;
    };
    class ChunkStreamer;   // the frame callback's chunk copies and deliveries (engine.cpp)
    bool generate_once(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                       const GenParams &gp, const UttParams *up, int32_t *codes, int *n_frames, FrameCb on_frames, void *user,
                       int interval, StreamState &st, bool *fault);
    class QueueStreamer;   // the queue callback's collections and deliveries (engine_queue.cpp)
    class QueueLoop;       // one run of the queue: the scheduler objects of queue_sched.h and the HIP calls they ask for
    // the records and prompt lengths of a call, validated: up's own, or (up null) the call-wide gp for every utterance
    bool resolve_utt_params(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                            const GenParams &gp, const UttParams *up, std::vector<UttParams> &ups, std::vector<int> &plen);
    // host scratch kept across calls (a per-call hipFree / hipHostFree synchronises the whole device)
    struct PinnedChunk { size_t cap = 0; int32_t *codes = nullptr; hipEvent_t ev = nullptr; };
    std::vector<PinnedChunk> chunk_pool_;   // streaming chunks of generate() and of the queue's deliveries
    bool pinned_chunk(size_t idx, size_t bytes, PinnedChunk **out);   // chunk_pool_[idx], grown to bytes, with its event
    void *pin_ = nullptr, *qout_ = nullptr, *qstage_ = nullptr;
    size_t pin_cap_ = 0, qout_cap_ = 0, qstage_cap_ = 0;
    bool ensure_pinned(size_t bytes);
    // device scratch p grown to bytes: qout_ (the queue's finished codes) and qstage_ (the queue deliveries' staging
    // chunk [S][interval][16] + header [S] + error word)
    bool ensure_device(void *&p, size_t &cap, size_t bytes);
    bool enqueue_talker_step(int S, hipStream_t s);
    bool enqueue_talker(int S, hipStream_t s, bool gather_input, bool select_next, bool prenormed = false,
                        bool *fold_advance = nullptr);
    bool talker_persist_one(hipStream_t s, bool gather_input, bool select_next, bool *fold_advance);
    bool talker_persist_batched(int S, hipStream_t s, bool gather, bool select_next);
    bool talker_per_op(int S, hipStream_t s, bool gather_input, bool select_next, bool prenormed);
    SelectSpec select_spec(int mode, const GenParams &gp, int frame_offset, int step) const;
    bool enqueue_cp_frame(int S, hipStream_t s, float *logits_host = nullptr, bool talker_next = false);
    bool cp_frame_persist_one(hipStream_t s);
    bool cp_frame_persist_batched(int S, hipStream_t s, bool talker_next);
    bool cp_frame_per_op(int S, hipStream_t s, float *logits_host, bool talker_next);
    // the pieces of one launch-per-op code-predictor pass around its stack and head
    bool cp_pass_input(int p, int S, bool defer, struct StackInput &in0, hipStream_t s);
    bool cp_copy_logits(int S, int step, float *logits_host, hipStream_t s);
    bool cp_select_handoff(int S, int step, hipStream_t s);
    // the three activation sets of the launch-per-op stacks, and the caches of the talker / code-predictor pass p
    StackBufs talker_bufs() const { return {x_, parts_, qkv_, xn_, attn_, hmlp_}; }
    StackBufs cp_bufs() const { return {cpx_, parts_, qkv_, xn_, attn_, hmlp_}; }
    StackBufs prefill_bufs() const { return {pf_x_, pf_parts_, pf_qkv_, pf_xn_, pf_attn_, pf_hmlp_}; }
    StackCache talker_cache() const;
    StackCache cp_cache(int p) const;
    GatherSum step_embed_gather() const;     // the talker step embedding of the frame's 16 codes
    GatherSum cp_input_gather(int p) const;   // code-predictor pass p >= 1: the table row of code p - 1
    // that table's first row in cp_qkvtab_ / cp_projtab_
    size_t cp_table_row0(int p) const { return p == 1 ? 0 : (size_t)c_.codec_vocab + (size_t)(p - 2) * c_.cp_vocab; }
    bool enqueue_frame(int S, hipStream_t s);
    bool enqueue_text_projection(int n_rows, hipStream_t s, const PromptScratch &ps);
    // the same over ids / scratch named one by one.  as_admission: the rows of an admission batch, whatever n_rows is (an
    // admission projects >= 7 rows, so it runs the matrix-core GEMM whenever that is on; a feed of one row must too)
    bool enqueue_text_projection(int n_rows, hipStream_t s, const int *idx, uint16_t *h, float *out, bool as_admission);
    // the prompt rows (PromptScratch::rows), trailing-text rows and pad row of every entry, assembled on stream s;
    // plen: each entry's prompt length in rows (prompt_len), trailing_len: per entry
    bool assemble_prompts(PromptScratch &ps, hipStream_t s, const std::vector<PromptEntry> &in, std::vector<int> &plen,
                          std::vector<int> &trailing_len);
    static int prompt_len(int language_id, bool has_spk);
    bool alloc_prompt_scratch(PromptScratch &ps, float *spk);
    // the checks shared by generate() and generate_queue(); plen: the prompt length
    bool check_gen_args(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                        const GenParams &gp, int *plen);
    // the same with a record per utterance: every record is validated before anything runs; ups: the records with
    // max_len resolved, plen: per utterance; id0: the id the messages give utterance 0 (an arrival's)
    bool check_utt_args(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                        const GenParams &gp, const UttParams *up, std::vector<UttParams> &ups, std::vector<int> &plen,
                        int id0 = 0);
    void set_gen_params(const GenParams &gp);   // gp_ = gp; drops the frame graphs that baked other sampling values
    // per-utterance sampling: the [max_slots] records the batched selections read while rec_on_ (select_spec); a one-slot
    // run leaves it off and bakes its utterance's values into the scalars (set_gen_params)
    SelRec *sel_rec_ = nullptr;
    bool rec_on_ = false;
    int *slot_max_len_ = nullptr;   // [max_slots] each slot's own max_len (queue deliveries), written while own_max_len_
    bool own_max_len_ = false;      // the running queue has a record per utterance
    static SelRec sel_rec(const UttParams &u) { return SelRec{u.temperature, u.top_k, u.rep_penalty, 0}; }
    // frame-graph cache key: graphs captured with and without the record pointer are both kept
    int frame_key(int key) const { return key + (rec_on_ ? (1 << 30) : 0); }
    template <class F> hipGraphExec_t capture(hipStream_t s, F &&enqueue);   // null with the error set
    bool graph_for(std::map<int, hipGraphExec_t> &cache, int S, bool (Engine::*fn)(int, hipStream_t));
    bool graph_for_key(std::map<int, hipGraphExec_t> &cache, int key, int S, bool (Engine::*fn)(int, hipStream_t));
    int policy_slots_ = 0;         // > 0: the batched stacks choose kernels as for this many slots (queue graphs)
    bool set_slot_state(int S, const std::vector<int> &pos, const std::vector<int> &frame);
    // causal prefill (one pass over the prompt rows of n_utt utterances, K/V written into slots pf_slot_[u])
    bool ensure_prefill();
    bool enqueue_prefill_rows(int S_main, int n_utt, int plen, int rows, hipStream_t s);   // plen 0: the ragged form
    bool prefill(int n_utt, int plen, const float *src, int S_main, hipStream_t s);
    // ragged form: src holds the packed rows; lens[u] in [1, 10].  pf_off_ / pf_len_ are filled from ps.rag_host
    bool prefill_ragged(int n_utt, const int *lens, const float *src, int S_main, hipStream_t s, PromptScratch &ps);
    std::map<int, hipGraphExec_t> g_prefill_;
    std::map<long long, hipGraphExec_t> g_prefill_rag_;   // key: (family, n_utt, total rows)
    int *pf_off_ = nullptr, *pf_len_ = nullptr;           // [max_slots] beside pf_slot_
    float *pf_x_ = nullptr, *pf_qkv_ = nullptr, *pf_parts_ = nullptr, *pf_hid_ = nullptr, *pf_logits_ = nullptr;
    uint16_t *pf_xn_ = nullptr, *pf_attn_ = nullptr, *pf_hmlp_ = nullptr;
    int *pf_slot_ = nullptr, *slot_iota_ = nullptr;
    // continuous batching: admission batches on their own stream (their prefill on the prefill scratch), then
    // activation of each slot on the main stream between two frames
    bool alloc_admission();
    bool admit_batch(const std::vector<int> &tgt, const std::vector<int> &utt, const int32_t *const *tokens,
                     const int *n_tokens, const float *const *speaker, const std::vector<UttParams> &ups,
                     const std::vector<int> &plen, bool ragged, hipStream_t as, int *tgt_h, std::vector<int> &trailing_len);
    bool activate_slot(int slot, uint64_t utt, int trailing_len, int n_tok, const UttParams &up, int plen, int *state_h,
                       bool deliveries = false);
    // text feeds: the round's descriptors travel in one pinned blob (a ring: a blob is rewritten only after the copy
    // that read it has run) to one device blob; hold_save_ keeps the hidden rows of held slots
    struct FeedScratch {
        static constexpr int NBUF = 4;
        int *pin[NBUF] = {};
        hipEvent_t e0[NBUF] = {}, e1[NBUF] = {};
        bool used[NBUF] = {};
        int *dev = nullptr, *error = nullptr;
        size_t cap_ints = 0;
        int cap_rows = 0, next = 0;
        TextRound round;   // the round being built (reserved once)
    } feed_;
    float *hold_save_ = nullptr;   // [max_slots][H]
    int *held_flag_ = nullptr;     // [max_slots] device: the slot is held (k_slot_hold)
    bool ensure_text_feed();
    bool enqueue_text_round(int S);   // feed_'s round, on the main stream
    bool retire_text_round(int b);    // ring blob b, if in use: wait for its round; its time into text_stats
    bool drain_text_rounds();         // the same for every round in flight, oldest first
    hipStream_t astream_ = nullptr;
    int *delivered_ = nullptr, *qmask_ = nullptr;   // queue deliveries: per-slot frames collected so far; a collection's slot mask
    float *ahidden_ = nullptr, *alogits_ = nullptr;
    int q_slots_ = 0;            // slot count of the running queue (the batch the admissions reproduce)

    Config c_;
    Config cpc_;                         // the code predictor's layer geometry (c_ with the cp_* values)
    bool mm_ok_ = true;                  // the batched matrix-core stack supports this model's shapes
    int fam1_ = 0;                       // !mm_ok_: every projection runs the vector kernels with a 1-slot K split
    bool use_mm(int S) const { return mm_ok_ && S >= gemm_mfma_min_batch(); }
    uint16_t *mtp_ = nullptr;            // code_pred.mtp_proj [cp_hidden][hidden] (1.7B)
    float *mtp_b_ = nullptr;             // its bias (optional)
    bool cp_project(int S, const float *x_talker, int ldx, hipStream_t s);   // cpx_ = mtp_proj . x + b
    std::string tts_path_, tok_path_;
    bool talker_ = true;   // false: vocoder-only context
    int device_ = 0, max_slots_ = 0, max_ctx_ = 0, max_trailing_ = 0;
    hipStream_t stream_ = nullptr;
    std::vector<void *> allocs_;
    WeightArena wa_;
    template <class T> T *dalloc(size_t n);

    // weights
    std::vector<DevLayer> L_, CP_;
    uint16_t *text_embd_ = nullptr, *fc1_ = nullptr, *fc2_ = nullptr, *codec_embd_ = nullptr, *codec_head_ = nullptr;
    float *fc1_b_ = nullptr, *fc2_b_ = nullptr, *out_norm_ = nullptr, *cp_out_norm_ = nullptr;
    std::vector<uint16_t *> cp_embd_, cp_head_;
    uint16_t **tabs16_dev_ = nullptr;   // codec_embd + code_pred.codec_embd[0..14]
    float *rope_ = nullptr;
    int rope_len_ = 0;

    // activations / state (sized for max_slots)
    float *x_ = nullptr, *qkv_ = nullptr, *logits_ = nullptr, *hidden_ = nullptr, *cpx_ = nullptr, *cp_in1_ = nullptr;
    float *cp_logits_ = nullptr, *part_ = nullptr;
    unsigned *ticket_ = nullptr;   // split-attention arrival counters [S][n_kv]
    unsigned *sel_ticket_ = nullptr;   // fused head+select arrival counters [S]
    uint16_t *attn_ = nullptr, *hmlp_ = nullptr;
    uint16_t *xn_ = nullptr;      // batched path: normalised f16 activations (resid_norm output)
    uint16_t *mtp_in_ = nullptr;  // batched path, 1.7B: the f16 talker rows code_pred.mtp_proj reads in pass 0
    float *parts_ = nullptr;      // batched path: split-K partial slabs [4][S][H]
    uint16_t *kc_ = nullptr, *vc_ = nullptr, *cpkc_ = nullptr, *cpvc_ = nullptr;
    int *pos_ = nullptr, *frame_ = nullptr, *done_ = nullptr, *token_ = nullptr, *tokens_ = nullptr;
    int *n_tokens_ = nullptr, *force_ = nullptr, *trailing_len_ = nullptr, *cp_pos_ = nullptr;
    uint8_t *seen_ = nullptr;
    uint64_t *utt_ = nullptr;
    uint64_t *seed_dev_ = nullptr;   // the sampling seed read by the captured selections (SelectSpec::seed_dev)
    uint64_t seed_host_ = 0;
    bool set_seed(uint64_t seed, hipStream_t s);
    float *trailing_ = nullptr, *tts_pad_ = nullptr;
    int32_t *codes_ = nullptr;
    int codes_max_len_ = 0;
    // prompt assembly scratch: the main stream's (its speaker rows are cp_in1_, which the main stream's frames reuse
    // after the prompt is assembled) and the admission stream's (alloc_admission: speaker rows of its own, the frame
    // loop of a model with mtp_proj writes cp_in1_ while an admission runs)
    PromptScratch main_ps_, adm_ps_;
    GenParams gp_;   // parameters baked into the captured frame graph
    Options opt_;
    int poll_every_ = 16;
    bool fused_select_ = true;
    bool cp_fused_attn_ = true;
    bool defer_cp_select_ = true;
    bool persist_ = true;
    bool persist_fallback_ = false;   // persistent kernels disabled after a flagged fault
    PLayerW *pl_dev_ = nullptr, *pl_cp_dev_ = nullptr;
    const uint16_t **heads_dev_ = nullptr;
    float *cp_qkvtab_ = nullptr;         // persistent code-predictor frame: layer 0's QKV row per table token
    float *cp_projtab_ = nullptr;        // 1.7B: mtp_proj . f16(table row) + b per table token (f32, code-predictor space)
    std::shared_ptr<struct CpTables> cp_tables_;   // the two tables above, shared by every context of this device
                                                   // that loaded the same weight file (engine.cpp, table registry)
    bool build_cp_proj_table();
    bool build_cp_qkv_table();
    bool build_persist_tables();
    bool tables_built_ = false;
    bool persist_cp_ = false;
    bool cp_roles_ = false;    // the 1-slot code-predictor frame runs persist_cp.hip
    bool tk_roles_ = false;    // the 1-slot talker step runs persist_tk.hip
    bool cpb_ = false;         // the batched code-predictor frame runs persist_cpb.hip (use_cpb)
    uint8_t *cpb_state_ = nullptr;
    bool setup_cpb(int n_cu);
    bool use_cpb(int S) const;
    bool tkb_ = false;         // the batched talker step runs persist_tkb.hip (use_tkb)
    uint8_t *tkb_state_ = nullptr;
    bool setup_tkb(int n_cu);
    bool use_tkb(int S) const;
    uint8_t *pstate_ = nullptr;
    int *table_iota_ = nullptr;   // 0..codec_vocab-1: the table builds' token ids
    uint64_t *pprof_ = nullptr;   // Q3T_DEV + Q3T_PERSIST_PROF: persistent-step timeline

    bool enqueue_cp_only(int S, hipStream_t s) { return enqueue_cp_frame(S, s); }
    std::map<int, hipGraphExec_t> g_talker_, g_frame_, g_cp_;
    std::unique_ptr<Vocoder> voc_;
    std::unique_ptr<SpeakerEncoder> spk_;
};

}  // namespace q3t
