// engine_queue.cpp — continuous batching (Engine::generate_queue): admission batches, slot activation, the
// queue's deliveries, text feeds and the loop that drives them.  The host decisions are queue_sched.h's and
// queue_deliver.h's; this file issues the HIP calls for them.
#include <climits>
#include <cstring>

#include "devlock.h"
#include "engine_internal.h"

namespace q3t {

// ------------------------------------------------------------------------------------------ continuous batching
// Admissions run on their own stream with private scratch, overlapping the frame loop of the other slots (at many
// slots the decode step leaves most of the chip idle).  The slots freed since the last admission are admitted
// together: their prompts are projected in one pass and run through ONE causal prefill (Engine::prefill), which
// writes the K/V rows [0, plen) of the target slots directly.  A target slot is parked in the frame loop meanwhile
// (done >= 0: no selection, no advance, its position >= plen): the frame graph still runs it, but writes only its own
// x / hidden / logits rows and the KV row at its parked position, none of which the admission writes.  The slot joins
// the frame loop (activate_slot, main stream, between two frames) once its admission batch has finished.  The prefill
// runs the running batch's kernels (S_main = q_slots_), whose per-row arithmetic does not depend on the other rows: a
// slot's prefill is what generate()'s prefill computes for it, whichever slots were admitted alongside.
bool Engine::alloc_admission() {
    if (astream_) return true;
    const int S = max_slots_, H = c_.hidden;
    if (!ensure_prefill()) return false;
    ahidden_ = dalloc<float>((size_t)S * H);
    alogits_ = dalloc<float>((size_t)S * c_.codec_vocab);
    delivered_ = dalloc<int>(S);
    qmask_ = dalloc<int>(S);
    if (!alloc_prompt_scratch(adm_ps_, nullptr)) return false;
    if (!ahidden_ || !alogits_ || !delivered_ || !qmask_) { set_error("device allocation failed"); return false; }
    // every buffer was zeroed on stream_ and drained by dalloc before the admission stream exists
    Q3T_HIP(hipStreamCreateWithFlags(&astream_, hipStreamNonBlocking));
    return true;
}

// admission batch on stream `as`: utterances utt[j] into slots tgt[j] (text projection, prefill / trailing / pad
// rows, the causal prefill into the target slots, hidden / logits rows per target slot).  tgt_h: pinned
// copy of tgt (alive until the batch has run); trailing_len[j]: the slot's trailing-text length
bool Engine::admit_batch(const std::vector<int> &tgt, const std::vector<int> &utt, const int32_t *const *tokens,
                         const int *n_tokens, const float *const *speaker, const std::vector<UttParams> &ups,
                         const std::vector<int> &plen, bool ragged, hipStream_t as, int *tgt_h,
                         std::vector<int> &trailing_len) {
    const int H = c_.hidden, a = (int)tgt.size();
    std::vector<PromptEntry> in(a);
    std::vector<int> lens(a), got;
    for (int j = 0, row = 0; j < a; row += lens[j], ++j) {
        lens[j] = plen[utt[j]];
        in[j] = PromptEntry{tokens[utt[j]], n_tokens[utt[j]], speaker ? speaker[utt[j]] : nullptr, tgt[j], ragged ? row : j * 10,
                            ups[utt[j]].language_id};
    }
    if (!assemble_prompts(adm_ps_, as, in, got, trailing_len)) return false;
    if (got != lens) { set_error("admit_batch: prefill length mismatch"); return false; }
    // the causal prefill of the batch with the running batch's kernels (S_main = q_slots_), K/V straight into the
    // target slots' rows [0, plen)
    for (int j = 0; j < a; ++j) tgt_h[j] = tgt[j];
    Q3T_HIP(hipMemcpyAsync(pf_slot_, tgt_h, a * 4, hipMemcpyHostToDevice, as));
    if (ragged ? !prefill_ragged(a, lens.data(), adm_ps_.rows, q_slots_, as, adm_ps_) : !prefill(a, lens[0], adm_ps_.rows, q_slots_, as))
        return false;
    const int V = c_.codec_vocab;
    for (int j = 0; j < a; ++j) {
        const size_t r = (ragged ? (size_t)in[j].row : (size_t)j * lens[0]) + lens[j] - 1;
        Q3T_HIP(hipMemcpyAsync(ahidden_ + (size_t)tgt[j] * H, pf_hid_ + r * H, H * 4, hipMemcpyDeviceToDevice, as));
        Q3T_HIP(hipMemcpyAsync(alogits_ + (size_t)tgt[j] * V, pf_logits_ + r * V, (size_t)V * 4, hipMemcpyDeviceToDevice, as));
    }
    return true;
}

// slot k joins the frame loop (main stream, between two frames, after its admission batch): per-slot state, the
// last prefill step's hidden state, and the CB0 of its first frame selected from the last prefill logits.
// state_h: pinned [16]
bool Engine::activate_slot(int k, uint64_t utt, int trailing_len, int n_tok, const UttParams &up, int plen, int *state_h,
                           bool deliveries) {
    const int H = c_.hidden, NCB = 16;
    state_h[0] = trailing_len; state_h[1] = n_tok; state_h[2] = up.force_frames; state_h[3] = -1;
    state_h[4] = plen; state_h[5] = 0;
    std::memcpy(state_h + 6, &utt, 8);
    state_h[8] = up.max_len;
    const SelRec rec = sel_rec(up);
    std::memcpy(state_h + 12, &rec, sizeof rec);
    if (own_max_len_) Q3T_HIP(hipMemcpyAsync(slot_max_len_ + k, state_h + 8, 4, hipMemcpyHostToDevice, stream_));
    if (rec_on_) Q3T_HIP(hipMemcpyAsync(sel_rec_ + k, state_h + 12, sizeof rec, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(trailing_len_ + k, state_h + 0, 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(n_tokens_ + k, state_h + 1, 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(force_ + k, state_h + 2, 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(utt_ + k, state_h + 6, 8, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemsetAsync(seen_ + (size_t)k * c_.codec_vocab, 0, c_.codec_vocab, stream_));
    Q3T_HIP(hipMemsetAsync(codes_ + (size_t)k * codes_max_len_ * NCB, 0, (size_t)codes_max_len_ * NCB * 4, stream_));
    Q3T_HIP(hipMemcpyAsync(hidden_ + (size_t)k * H, ahidden_ + (size_t)k * H, H * 4, hipMemcpyDeviceToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(pos_ + k, state_h + 4, 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(frame_ + k, state_h + 5, 4, hipMemcpyHostToDevice, stream_));
    if (deliveries) Q3T_HIP(hipMemsetAsync(delivered_ + k, 0, 4, stream_));   // queue deliveries: nothing collected yet
    Q3T_HIP(hipMemcpyAsync(done_ + k, state_h + 3, 4, hipMemcpyHostToDevice, stream_));
    SelectSpec sp = select_spec(SEL_CB0, gp_, 0, 0);   // the slot's rows of every per-slot array
    sp.tokens += (size_t)k * 16; sp.codes += (size_t)k * codes_max_len_ * NCB; sp.frame += k; sp.done += k; sp.utt += k;
    sp.seen += (size_t)k * c_.codec_vocab; sp.n_tokens += k; sp.force_frames += k;
    if (sp.ticket) sp.ticket += k;
    if (sp.rec) sp.rec += k;
    return select_tokens(sp, alogits_ + (size_t)k * c_.codec_vocab, 1, stream_);
}

// Deliveries of generate_queue() (DESIGN 2f "Queue deliveries").  A collection is ONE k_queue_collect launch over the
// slots of a mask, one copy of the staging chunk (rows, header, error word) into a pinned chunk of the context's pool
// and one event.  The device keeps each slot's collected-frames counter, so the host uploads the mask and nothing
// else.  Chunks are delivered in stream order, a tick's chunk one tick late and a finish chunk one frame late, so
// the GPU runs the queued frames during the callback; each is handed out only once the persistent kernels behind it
// are known to be fault-free.
class Engine::QueueStreamer {
public:
    // own_max_len: a collection clamps each slot's frames to its own max_len (slot_max_len_) as well
    // alog (the open queue): the utterance indices are handles of the arrival log, and the callback is given their ids
    QueueStreamer(Engine &e, int S, int n_utt, int max_len, bool own_max_len, QueueCb cb, void *user, int interval,
                  QueueState &st, bool *fault, const ArrivalLog *alog = nullptr)
        : e_(e), S_(S), max_len_(max_len), interval_(interval), own_max_len_(own_max_len), cb_(cb), user_(user), st_(st),
          fault_(fault), alog_(alog), run_(n_utt) {}
    // the open queue: the per-utterance tables have n rows now; the chunks collected / delivered so far (a handle is
    // reused only when no pending chunk can name it: retire_arrivals)
    void grow(size_t n) { run_.run.resize(n, 0); run_.gone.resize(n, 0); }
    QueueRun &run() { return run_; }
    bool pending() const { return !pend_.empty(); }
    size_t collected() const { return n_collected_; }
    size_t delivered() const { return n_delivered_; }
    bool active() const { return cb_ != nullptr; }
    int interval() const { return interval_; }
    bool begin() {   // the staging chunk with a clear error word
        if (!e_.ensure_device(e_.qstage_, e_.qstage_cap_, stage_ints() * 4)) return false;
        Q3T_HIP(hipMemsetAsync(static_cast<int *>(e_.qstage_) + stage_ints() - 1, 0, 4, e_.stream_));
        return true;
    }
    // one collection over the slots k with sel[k] != 0 (slot_utt[k]: the slot's utterance), queued behind what the
    // stream holds; its chunk is due when the loop clock reaches `due`
    bool collect(const std::vector<int> &slot_utt, const std::vector<char> &sel, bool final, int due) {
        Chunk c;
        if (!pool_.empty()) { c = pool_.back(); pool_.pop_back(); }
        else {
            PinnedChunk *pc = nullptr;   // rows [S][interval][16], header [S], error word, then the mask's source [S]
            if (!e_.pinned_chunk(next_chunk_++, (stage_ints() + S_) * 4, &pc)) return false;
            c.rows = pc->codes;
            c.ev = pc->ev;
        }
        c.final = final;
        c.due = due;
        c.utt.assign(S_, -1);
        int *mask = c.rows + stage_ints();
        for (int k = 0; k < S_; ++k) {
            mask[k] = sel[k] ? 1 : 0;
            if (sel[k]) c.utt[k] = slot_utt[k];
        }
        int32_t *stage = static_cast<int32_t *>(e_.qstage_);
        Q3T_HIP(hipMemcpyAsync(e_.qmask_, mask, S_ * 4, hipMemcpyHostToDevice, e_.stream_));
        QueueCollect q;
        q.mask = e_.qmask_; q.done = e_.done_; q.frame = e_.frame_; q.delivered = e_.delivered_;
        q.codes = e_.codes_;
        q.rows = stage;
        q.header = stage + (size_t)S_ * interval_ * NCB;
        q.error = stage + stage_ints() - 1;
        q.interval = interval_; q.codes_max_len = e_.codes_max_len_; q.max_len = max_len_;
        if (own_max_len_) q.slot_max_len = e_.slot_max_len_;
        if (!queue_collect(q, S_, e_.stream_)) return false;
        Q3T_HIP(hipMemcpyAsync(c.rows, stage, stage_ints() * 4, hipMemcpyDeviceToHost, e_.stream_));
        Q3T_HIP(hipEventRecord(c.ev, e_.stream_));
        pend_.push_back(c);
        ++n_collected_;
        return true;
    }
    // the pending chunks up to the last one due at loop clock f, oldest first
    bool deliver_due(int f) {
        size_t n = 0;
        for (size_t i = 0; i < pend_.size(); ++i)
            if (pend_[i].due <= f) n = i + 1;
        for (size_t i = 0; i < n && !st_.aborted; ++i) {
            Chunk c = pend_.front();
            pend_.erase(pend_.begin());
            pool_.push_back(c);
            ++n_delivered_;
            if (!deliver(c)) { hipStreamSynchronize(e_.stream_); return false; }
        }
        return true;
    }
    bool flush() { return deliver_due(INT_MAX); }
    // utterances the callback cancelled since the last call (their slots are still running)
    std::vector<int> take_stops() { std::vector<int> s; s.swap(stops_); return s; }

private:
    static constexpr int NCB = 16;
    struct Chunk { int32_t *rows = nullptr; hipEvent_t ev = nullptr; bool final = false; int due = 0; std::vector<int> utt; };
    size_t stage_ints() const { return (size_t)S_ * interval_ * NCB + S_ + 1; }
    bool deliver(const Chunk &c) {
        Q3T_HIP(hipEventSynchronize(c.ev));
        if (e_.persist_error()) { *fault_ = true; return false; }
        const int *hdr = c.rows + (size_t)S_ * interval_ * NCB;
        if (hdr[S_] != 0) { set_error("generate_queue: a collection was out of step with its slot"); return false; }
        // (a fallback re-run generates every utterance again: queue_deliver.h keeps what was handed out apart)
        std::vector<QueueEntry> ent;
        queue_plan(hdr, c.utt, c.final, st_, run_, ent, stops_);
        if (ent.empty()) return true;
        if (alog_)   // handles are reused: increasing id is not increasing handle
            std::sort(ent.begin(), ent.end(), [this](const QueueEntry &a, const QueueEntry &b) { return alog_->e[a.utt].id < alog_->e[b.utt].id; });
        const size_t m = ent.size();
        std::vector<int32_t> utt(m), nf(m), fin(m), stop(m, 0);
        std::vector<const int32_t *> cp(m);
        for (size_t i = 0; i < m; ++i) {
            utt[i] = alog_ ? alog_->e[ent[i].utt].id : ent[i].utt; nf[i] = ent[i].n; fin[i] = ent[i].final;
            cp[i] = c.rows + ((size_t)ent[i].slot * interval_ + ent[i].skip) * NCB;
        }
        const int go = cb_(user_, (int32_t)m, utt.data(), cp.data(), nf.data(), fin.data(), stop.data());
        queue_commit(ent, stop.data(), go != 0, st_, run_, stops_);
        return true;
    }
    Engine &e_;
    const int S_, max_len_, interval_;
    const bool own_max_len_;
    const QueueCb cb_;
    void *const user_;
    QueueState &st_;
    bool *const fault_;
    const ArrivalLog *const alog_;
    size_t n_collected_ = 0, n_delivered_ = 0;
    QueueRun run_;                    // this run's per-utterance progress (queue_deliver.h)
    std::vector<int> stops_;          // utterances to cancel: their slots may still be running
    size_t next_chunk_ = 0;           // chunk_pool_[0, next_chunk_) are in use by this call
    std::vector<Chunk> pend_, pool_;  // collections in flight, oldest first; chunks delivered and free for reuse
};

// Text feeds (DESIGN 2f "Text feeds").  A round (feed_.round, a TextRound built by queue_sched.h's TextPlanner) is what
// the asks of one loop iteration produced.  It travels as ONE pinned blob -> ONE device blob (TextRound::pack) on the
// main stream, followed by the text projection over all ids, one k_text_append and at most one hold and one release
// launch.
bool Engine::ensure_text_feed() {
    FeedScratch &F = feed_;
    if (F.dev) return true;
    const int S = max_slots_;
    F.cap_rows = S * max_trailing_ + 1;
    F.cap_ints = (size_t)5 * S + (size_t)4 * F.cap_rows;
    if (F.cap_rows > main_ps_.cap) { set_error("text feeds: projection scratch too small"); return false; }
    int *dev = dalloc<int>(F.cap_ints + 1);
    hold_save_ = dalloc<float>((size_t)S * c_.hidden);
    held_flag_ = dalloc<int>(S);
    if (!dev || !hold_save_ || !held_flag_) { set_error("device allocation failed"); return false; }
    for (int b = 0; b < FeedScratch::NBUF; ++b) {
        Q3T_HIP(hipHostMalloc(reinterpret_cast<void **>(&F.pin[b]), F.cap_ints * 4, hipHostMallocDefault));
        Q3T_HIP(hipEventCreate(&F.e0[b]));
        Q3T_HIP(hipEventCreate(&F.e1[b]));
    }
    F.round.reserve(F.cap_rows, S);
    F.error = dev + F.cap_ints;   // zeroed by dalloc
    F.dev = dev;
    return true;
}

bool Engine::retire_text_round(int b) {
    FeedScratch &F = feed_;
    if (!F.used[b]) return true;
    F.used[b] = false;
    Q3T_HIP(hipEventSynchronize(F.e1[b]));
    float ms = 0;
    Q3T_HIP(hipEventElapsedTime(&ms, F.e0[b], F.e1[b]));
    text_stats.feed_ms += ms;
    return true;
}

bool Engine::drain_text_rounds() {
    for (int i = 0; i < FeedScratch::NBUF; ++i)
        if (!retire_text_round((feed_.next + i) % FeedScratch::NBUF)) return false;   // oldest first
    return true;
}

bool Engine::enqueue_text_round(int S) {
    FeedScratch &F = feed_;
    const TextRound &R = F.round;
    const int b = F.next;
    F.next = (b + 1) % FeedScratch::NBUF;
    // the round that last used this blob: long since run, unless the host is NBUF rounds ahead
    if (!retire_text_round(b)) return false;
    if ((int)R.ids.size() > F.cap_rows || (int)R.rows.size() / 3 > F.cap_rows || (int)R.commit.size() / 3 > S ||
        (int)R.hold.size() != S || (int)R.rel.size() != S) {
        set_error("text feeds: round larger than its scratch");
        return false;
    }
    const TextRound::Layout l = R.pack(F.pin[b], S);
    Q3T_HIP(hipEventRecord(F.e0[b], stream_));
    Q3T_HIP(hipMemcpyAsync(F.dev, F.pin[b], l.ints * 4, hipMemcpyHostToDevice, stream_));
    if (l.n_ids && !enqueue_text_projection(l.n_ids, stream_, F.dev + l.o_ids, main_ps_.h, main_ps_.out, true)) return false;
    TextAppend t;
    t.src = main_ps_.out; t.trailing = trailing_; t.rows = F.dev + l.o_rows; t.commit = F.dev + l.o_commit;
    t.trailing_len = trailing_len_; t.n_tokens = n_tokens_; t.error = F.error;
    t.n_rows = l.n_rows; t.n_commit = l.n_commit; t.src_rows = l.n_ids; t.S = S; t.max_trailing = max_trailing_; t.H = c_.hidden;
    if (!text_append(t, stream_)) return false;
    SlotHold h;
    h.hidden = hidden_; h.save = hold_save_; h.done = done_; h.held = held_flag_; h.frame = frame_; h.H = c_.hidden;
    h.mask = F.dev + l.o_rel;
    if (R.any_rel && !slot_release(h, S, stream_)) return false;
    h.mask = F.dev;
    if (R.any_hold && !slot_hold(h, S, stream_)) return false;
    Q3T_HIP(hipEventRecord(F.e1[b], stream_));
    F.used[b] = true;
    ++text_stats.feed_rounds;
    return true;
}


// One run of the queue (generate_queue starts a second one after a hand-off fault).  What to do is decided by the
// SlotTable and the TextPlanner of queue_sched.h; the member functions below issue the HIP calls for it and keep the
// call's handles: streams, pinned words, events and the QueueStreamer.
class Engine::QueueLoop {
public:
    QueueLoop(Engine &e, int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
              const GenParams &gp, const UttParams *up, int32_t *codes, int *n_frames, int max_active, QueueCb on_batch,
              void *user, int interval, QueueState &qst, const TextFeed *text, TextLog *tlog)
        : e_(e), n_utt_(n_utt), S_(std::min(e.max_slots_, n_utt)), max_active_(max_active <= 0 || max_active > S_ ? S_ : max_active),
          interval_(interval), tokens_in_(tokens), n_tokens_in_(n_tokens), tokens_(tokens), n_tokens_(n_tokens), speaker_(speaker),
          gp_(gp), up_(up), codes_(codes), n_frames_(n_frames), qst_(qst), text_(text), tlog_(tlog), dev_hold_(text && S_ > 1),
          qs_(e, S_, n_utt, gp.max_len, up != nullptr, on_batch, user, interval, qst, &fault_), t_(S_), tp_(n_utt), sel_(S_, 0),
          g1_(gp) {}
    // the open form (generate_queue_open): S slots whatever arrives, the records path, the ragged prefill
    QueueLoop(Engine &e, const GenParams &gp, int S, int max_active, ArriveCb arrive, QueueCb on_batch, void *user, int interval,
              QueueState &qst, ArrivalLog *alog)
        : e_(e), n_utt_(0), S_(S), max_active_(max_active <= 0 || max_active > S ? S : max_active), interval_(interval),
          tokens_in_(nullptr), n_tokens_in_(nullptr), tokens_(nullptr), n_tokens_(nullptr), speaker_(nullptr), gp_(gp), up_(nullptr),
          codes_(nullptr), n_frames_(nullptr), qst_(qst), text_(nullptr), tlog_(nullptr), dev_hold_(false),
          qs_(e, S, 0, gp.max_len, true, on_batch, user, interval, qst, &fault_, alog), t_(S), tp_(0), sel_(S, 0), g1_(gp),
          alog_(alog), arrive_(arrive), arrive_user_(user) {}
    bool run();
    bool run_open();
    bool faulted() const { return fault_; }   // run() failed on a persistent kernel's hand-off fault

private:
    static constexpr int NCB = 16;
    bool prepare();          // checks, scratch and the call's parameters: nothing a failure has to undo
    bool park_all();
    bool loop();
    bool finish();
    bool admit();
    bool activate();
    bool release(int k, bool park_slot);
    bool deliver(int due);
    bool reap();
    bool text_round();
    bool frame_graph(hipGraphExec_t *g);
    bool idle_round();
    bool wait_admission();
    bool poll();
    void one_slot_params(const UttParams &r);
    void restore_context();
    // the open form
    bool prepare_open();
    bool loop_open();
    bool arrivals();
    bool admit_open();
    bool retire();
    void sync_tables();
    void bind(int h);
    static std::string check_cb(void *ctx, int32_t id, const Arrival &a, UttParams *up, int *plen) {
        QueueLoop *q = static_cast<QueueLoop *>(ctx);
        return q->e_.check_arrival(id, a, q->gp_, up, plen);
    }

    Engine &e_;
    const int n_utt_, S_, max_active_, interval_;
    const int32_t *const *const tokens_in_;
    const int *const n_tokens_in_;
    const int32_t *const *tokens_;   // (open utterances: their heads padded, below)
    const int *n_tokens_;
    const float *const *speaker_;
    const GenParams &gp_;            // the call's (e_.gp_: what the captured frame graphs bake)
    const UttParams *const up_;
    int32_t *const codes_;
    int *n_frames_;
    QueueState &qst_;
    const TextFeed *const text_;
    TextLog *const tlog_;
    // text feeds on a slot that shares a frame graph with running ones: the device-side hold.  A one-slot context holds
    // by not launching (its persistent kernels own the device; nothing else would run)
    const bool dev_hold_;
    bool fault_ = false;
    QueueStreamer qs_;
    SlotTable t_;
    TextPlanner tp_;
    std::vector<char> sel_;
    GenParams g1_;                   // one slot with records: the utterance's values in the scalars (one_slot_params)
    std::vector<std::vector<int32_t>> head_pad_;
    std::vector<const int32_t *> tok_eff_;
    std::vector<int> nt_eff_;
    std::vector<UttParams> ups_;
    std::vector<int> plens_, cap_;   // per utterance: prompt rows, max_len
    std::vector<int> batch_tl_;      // the admission batch in flight: trailing-text lengths
    bool mixed_plen_ = false;
    int plen_ = 0;                   // where a free slot waits: above the rows any prefill of the call writes
    int fam_ = 0;                    // queue_family: the fewest slots a frame graph covers
    hipStream_t as_ = nullptr;       // the admissions' stream
    int32_t *out_dev_ = nullptr;     // the finished utterances' codes, copied to the caller once at the end
    int *pin_ = nullptr, *done_h_ = nullptr, *tgt_h_ = nullptr, *park_ = nullptr, *held_h_ = nullptr;
    Event aev_{hipEventDisableTiming}, pev_{hipEventDisableTiming}, rev_{hipEventDisableTiming};   // admission, poll, release
    int f_ = 0;                      // the loop clock: frame graphs launched
    bool polled_ = false;            // one frame in flight: frame f is launched before frame f-1's done flags are read
    // the open form: every per-utterance table above is indexed by the handles of the arrival log and grows with it
    ArrivalLog *const alog_ = nullptr;
    const ArriveCb arrive_ = nullptr;
    void *const arrive_user_ = nullptr;
    ArrivalPlanner ap_;
    std::vector<const float *> spk_eff_;
    std::vector<int> nf_;            // n_frames_ of the open form
    int f_mark_ = 0;                 // the loop clock at the last arrival, activation or release
};

bool Engine::QueueLoop::prepare() {
    Engine &e = e_;
    // open utterances (text feeds): a head [3 role ids, >= 1 text id] runs as the prompt head || five ids, whose rows
    // are exactly the head's (the five are dropped by plan_rows); its trailing row K0 = n_head - 4, the tts_eos row of
    // that prompt, is not counted while the text is open and is overwritten by the first feed
    if (text_) {
        tok_eff_.assign(tokens_in_, tokens_in_ + n_utt_);
        nt_eff_.assign(n_tokens_in_, n_tokens_in_ + n_utt_);
        head_pad_.resize(n_utt_);
        for (int u = 0; u < n_utt_; ++u) {
            if (!text_->open[u]) continue;
            const std::string err = open_head(u, tokens_in_[u], n_tokens_in_[u], e.c_.text_vocab, e.max_trailing_, e.c_.tts_pad, head_pad_[u]);
            if (!err.empty()) { set_error(err); return false; }
            tok_eff_[u] = head_pad_[u].data();
            nt_eff_[u] = n_tokens_in_[u] + 5;
        }
        tokens_ = tok_eff_.data();
        n_tokens_ = nt_eff_.data();
        if (!e.ensure_text_feed()) return false;
    }
    // the call-wide form: one record and one prompt length for every utterance.  With records (up): each utterance's own;
    // admission batches then pack their prompt rows and run the ragged prefill
    if (!e.resolve_utt_params(n_utt_, tokens_, n_tokens_, speaker_, gp_, up_, ups_, plens_)) return false;
    cap_.resize(n_utt_);
    for (int u = 0; u < n_utt_; ++u) {
        mixed_plen_ = mixed_plen_ || plens_[u] != plens_[0];
        cap_[u] = ups_[u].max_len;
    }
    plen_ = mixed_plen_ ? 10 : plens_[0];
    if (gp_.max_len > e.codes_max_len_) { set_error("max_len exceeds the code buffer"); return false; }
    if (!e.alloc_admission()) return false;
    e.q_slots_ = S_;
    // the single-slot context runs persistent kernels, which need the whole device: admissions go on the main stream
    as_ = (S_ == 1 && e.persist_enabled()) ? e.stream_ : e.astream_;
    e.rec_on_ = up_ && S_ > 1;
    e.own_max_len_ = up_ != nullptr;
    if (!up_) e.set_gen_params(gp_);
    if (!e.set_seed(gp_.seed, e.stream_)) return false;
    // the finished utterances' codes (device scratch kept by the context); a caller that takes deliveries may pass no
    // codes buffer: nothing is parked then
    if (codes_ && !e.ensure_device(e.qout_, e.qout_cap_, (size_t)n_utt_ * gp_.max_len * NCB * 4)) return false;
    out_dev_ = codes_ ? static_cast<int32_t *>(e.qout_) : nullptr;
    if (qs_.active() && !qs_.begin()) return false;
    // an aborted call copies out rows of utterances that never ran (and with records a release parks only the
    // utterance's own max_len rows)
    if ((qs_.active() || up_ || text_) && out_dev_)
        Q3T_HIP(hipMemsetAsync(out_dev_, 0, (size_t)n_utt_ * gp_.max_len * NCB * 4, e.stream_));
    // [S][16] activation staging, [S] done flags, [S] admission targets, the constants 0 (parking) and the waiting
    // position, [S] held flags (text feeds: polled beside the done flags): pinned, kept
    if (!e.ensure_pinned(((size_t)S_ * 19 + 2) * 4)) return false;
    pin_ = static_cast<int *>(e.pin_);
    done_h_ = pin_ + (size_t)S_ * 16; tgt_h_ = pin_ + (size_t)S_ * 17; park_ = pin_ + (size_t)S_ * 18;
    held_h_ = pin_ + (size_t)S_ * 18 + 2;
    for (int k = 0; k < S_; ++k) held_h_[k] = 0;
    park_[0] = 0;
    park_[1] = plen_;
    return true;
}

// every slot starts parked: done = 0 (no selection, no advance), position plen (above the rows a prefill writes),
// valid code ids for the gathers it still runs through, no trailing text
bool Engine::QueueLoop::park_all() {
    Engine &e = e_;
    std::vector<int> pl(S_, plen_);
    Q3T_HIP(hipMemsetAsync(e.done_, 0, S_ * 4, e.stream_));
    Q3T_HIP(hipMemcpyAsync(e.pos_, pl.data(), S_ * 4, hipMemcpyHostToDevice, e.stream_));
    Q3T_HIP(hipMemsetAsync(e.frame_, 0, S_ * 4, e.stream_));
    Q3T_HIP(hipMemsetAsync(e.tokens_, 0, (size_t)S_ * 16 * 4, e.stream_));
    Q3T_HIP(hipMemsetAsync(e.trailing_len_, 0, S_ * 4, e.stream_));
    if (text_) Q3T_HIP(hipMemsetAsync(e.held_flag_, 0, S_ * 4, e.stream_));
    Q3T_HIP(hipStreamSynchronize(e.stream_));
    return true;
}

// one slot with records: each utterance's values go into the scalars when it takes the slot
void Engine::QueueLoop::one_slot_params(const UttParams &r) {
    if (r.temperature == e_.gp_.temperature && r.top_k == e_.gp_.top_k && r.rep_penalty == e_.gp_.rep_penalty) return;
    hipStreamSynchronize(e_.stream_);   // the frame graphs about to be dropped may still run
    g1_.temperature = r.temperature; g1_.top_k = r.top_k; g1_.rep_penalty = r.rep_penalty;
    e_.set_gen_params(g1_);
}

bool Engine::QueueLoop::admit() {   // every free slot, up to max_active busy, one batch
    Engine &e = e_;
    std::vector<int> tgt, utt;
    t_.pick_admission(n_utt_, max_active_, tgt, utt);
    if (tgt.empty()) return true;
    if (mixed_plen_ && as_ != e.stream_) {
        // a released slot was moved to the waiting position on the main stream (release): the batch's prefill, which
        // may write more rows than the slot's last utterance had, starts behind that
        Q3T_HIP(hipEventRecord(rev_, e.stream_));
        Q3T_HIP(hipStreamWaitEvent(as_, rev_, 0));
    }
    if (!e.admit_batch(tgt, utt, tokens_, n_tokens_, speaker_, ups_, plens_, up_ != nullptr, as_, tgt_h_, batch_tl_)) return false;
    Q3T_HIP(hipEventRecord(aev_, as_));
    t_.admitted(tgt, utt, batch_tl_);
    return true;
}

bool Engine::QueueLoop::activate() {   // the batch in flight has finished: its slots join the frame loop
    Engine &e = e_;
    if (as_ != e.stream_) Q3T_HIP(hipStreamWaitEvent(e.stream_, aev_, 0));
    for (int k : t_.batch_tgt) {
        const int u = t_.slot_utt[k];
        if ((up_ || alog_) && S_ == 1) one_slot_params(ups_[u]);
        // an open utterance: its rows without the tts_eos row, n_tokens = K + 9 (what the padded head counts).  Sampling is
        // keyed by the utterance's index, in the open form by its arrival's key
        if (!e.activate_slot(k, alog_ ? alog_->e[u].key : (uint64_t)u, t_.tl[k] - (text_ && tp_.is_open[u] ? 1 : 0), n_tokens_[u], ups_[u], plens_[u],
                             pin_ + (size_t)k * 16, qs_.active()))
            return false;
        if (dev_hold_) Q3T_HIP(hipMemsetAsync(e.held_flag_ + k, 0, 4, e.stream_));
        t_.activated(k);
    }
    t_.batch_tgt.clear();
    return true;
}

// the frame graph over the slots SlotTable::frame_slots names, with the S-slot kernel family (policy_slots_ = S)
bool Engine::QueueLoop::frame_graph(hipGraphExec_t *g) {
    const int se = t_.frame_slots(fam_);
    const int key = e_.frame_key(se + 65536 * S_);
    if (!e_.graph_for_key(e_.g_frame_, key, se, &Engine::enqueue_frame)) return false;
    *g = e_.g_frame_[key];
    return true;
}

// an utterance leaves its slot (ended, or cancelled by the delivery callback): its codes are parked for the
// end-of-call copy and the slot is free for the next admission
bool Engine::QueueLoop::release(int k, bool park_slot) {
    Engine &e = e_;
    const int u = t_.slot_utt[k];
    if (out_dev_)
        Q3T_HIP(hipMemcpyAsync(out_dev_ + (size_t)u * gp_.max_len * NCB, e.codes_ + (size_t)k * e.codes_max_len_ * NCB,
                               (size_t)cap_[u] * NCB * 4, hipMemcpyDeviceToDevice, e.stream_));
    if (park_slot)   // still running: park the slot (no selection, no advance)
        Q3T_HIP(hipMemcpyAsync(e.done_ + k, park_, 4, hipMemcpyHostToDevice, e.stream_));
    if (dev_hold_ && t_.hheld[k]) Q3T_HIP(hipMemsetAsync(e.held_flag_ + k, 0, 4, e.stream_));   // (cancelled while held)
    if (mixed_plen_)   // its successor's prompt may be longer than the position it stopped at: back to the waiting one
        Q3T_HIP(hipMemcpyAsync(e.pos_ + k, park_ + 1, 4, hipMemcpyHostToDevice, e.stream_));
    t_.released(k);
    return true;
}

// the chunks due at loop clock `due`, then the slots of the utterances their callbacks cancelled
bool Engine::QueueLoop::deliver(int due) {
    if (!qs_.deliver_due(due)) return false;
    for (int u : qs_.take_stops()) {
        for (int k = 0; k < S_; ++k)
            if (t_.state[k] == SlotTable::ACTIVE && t_.slot_utt[k] == u && !release(k, true)) return false;
        // its length is what it was handed, also when it had ended (and left its slot) before the piece the
        // callback cancelled it at was delivered
        n_frames_[u] = qst_.delivered[u];
    }
    return true;
}

// the slots whose utterance ended by the polled flags (SlotTable::ended) leave their slots
bool Engine::QueueLoop::reap() {
    Q3T_HIP(hipEventSynchronize(pev_));
    const bool any = t_.ended(done_h_, held_h_, cap_, sel_);
    // the rest of the finished slots' frames, before a slot is parked or handed to a successor
    if (qs_.active() && any && !qs_.collect(t_.slot_utt, sel_, true, f_ + 1)) return false;
    for (int k = 0; k < S_; ++k) {
        if (!sel_[k]) continue;
        const int d = done_h_[k], u = t_.slot_utt[k];
        n_frames_[u] = frames_of(d, cap_[u]);
        if (!release(k, d < 0)) return false;   // d < 0: stopped at max_len
    }
    return true;
}

// text feeds: the asks of this iteration and the round they make (TextPlanner), on the main stream
bool Engine::QueueLoop::text_round() {
    bool aborted = false;
    const std::string err = tp_.ask(t_, text_->cb, text_->user, &aborted);
    if (!err.empty()) { set_error(err); return false; }
    if (aborted) { qst_.aborted = true; return true; }
    tp_.close_round(t_, cap_, text_->held);
    return e_.feed_.round.empty() || e_.enqueue_text_round(S_);
}

// every busy slot is held: launch nothing.  What the last poll shows, the pending deliveries (nothing runs behind
// them), an admission if one is in flight or possible, then ask again: waiting for text is the callback's job
bool Engine::QueueLoop::idle_round() {
    ++e_.text_stats.idle_rounds;
    if (polled_ && !reap()) return false;
    polled_ = false;
    if (qs_.active() && !deliver(INT_MAX)) return false;
    if (qst_.aborted) return true;
    if (t_.batch_tgt.empty() && t_.next < n_utt_ && !admit()) return false;
    if (!t_.batch_tgt.empty()) {
        Q3T_HIP(hipEventSynchronize(aev_));
        if (!activate()) return false;
    }
    return true;
}

// only an admission in flight: wait for it instead of running empty frames
bool Engine::QueueLoop::wait_admission() {
    if (qs_.active() && !deliver(INT_MAX)) return false;   // nothing runs behind them: hand out what is pending
    if (qst_.aborted) return true;
    if (t_.batch_tgt.empty() && !admit()) return false;
    Q3T_HIP(hipEventSynchronize(aev_));
    if (!activate()) return false;
    polled_ = false;
    return true;
}

// the done (and held) flags behind the frame just launched, read one frame late (reap)
bool Engine::QueueLoop::poll() {
    Engine &e = e_;
    Q3T_HIP(hipMemcpyAsync(done_h_, e.done_, S_ * 4, hipMemcpyDeviceToHost, e.stream_));
    if (dev_hold_) Q3T_HIP(hipMemcpyAsync(held_h_, e.held_flag_, S_ * 4, hipMemcpyDeviceToHost, e.stream_));
    t_.polled();
    Q3T_HIP(hipEventRecord(pev_, e.stream_));
    polled_ = true;
    return true;
}

bool Engine::QueueLoop::loop() {
    Engine &e = e_;
    while (t_.n_fin < n_utt_ && !qst_.aborted) {
        if (text_ && !text_round()) return false;
        if (qst_.aborted) break;
        const int n_active = t_.n_active();
        if (n_active > 0 && t_.n_run() == 0) { if (!idle_round()) return false; continue; }
        if (n_active == 0) { if (!wait_admission()) return false; continue; }
        hipGraphExec_t fg = nullptr;
        if (!frame_graph(&fg)) return false;
        if (!e.persist_fault_hook(S_, (e.persist_ ? 1 : 0) + (e.persist_cp_ ? 1 : 0))) return false;
        Q3T_HIP(hipGraphLaunch(fg, e.stream_));
        ++f_;
        t_.launched();
        if (text_) {
            ++e.text_stats.graph_launches;
            tp_.tick = f_ % interval_ == 0;
        }
        if (qs_.active()) {
            // a tick: the new frames of every active slot, behind this frame's graph; then the chunks due by now (the
            // previous tick's, and the finish chunks of the previous frame)
            if (f_ % qs_.interval() == 0) {
                for (int k = 0; k < S_; ++k) sel_[k] = t_.state[k] == SlotTable::ACTIVE;
                if (!qs_.collect(t_.slot_utt, sel_, false, f_ + qs_.interval())) return false;
            }
            if (!deliver(f_)) return false;
            if (qst_.aborted) break;
        }
        if (polled_ && !reap()) return false;   // done_h: after frame f-1
        if (!t_.batch_tgt.empty() && (as_ == e.stream_ || hipEventQuery(aev_) == hipSuccess) && !activate()) return false;
        if (t_.batch_tgt.empty() && t_.next < n_utt_ && !admit()) return false;
        if (as_ == e.stream_ && !t_.batch_tgt.empty() && !activate()) return false;
        if (!poll()) return false;
        if (queue_no_progress(f_, n_utt_, gp_.max_len, plen_)) { set_error("generate_queue: no progress"); return false; }
    }
    return true;
}

// after the loop: the last deliveries, the lengths of an aborted call, the feeds' error word, the codes
bool Engine::QueueLoop::finish() {
    Engine &e = e_;
    if (qs_.active()) {
        if (!qst_.aborted && !qs_.flush()) return false;   // the last finish chunks
        if (qst_.aborted) {   // the callback ended the call: every utterance is as long as what it was handed
            for (int k = 0; k < S_; ++k)
                if (t_.state[k] == SlotTable::ACTIVE && !release(k, false)) return false;
            for (int u = 0; u < n_utt_; ++u) n_frames_[u] = qst_.delivered[u];
        } else {
            for (int u = 0; u < n_utt_; ++u)
                if (qst_.stopped[u]) n_frames_[u] = qst_.delivered[u];   // (a re-run: cancelled before the fault)
            for (int u = 0; u < n_utt_; ++u)
                if (!(qst_.stopped[u] || (qst_.finaled[u] && qst_.delivered[u] == n_frames_[u]))) {
                    set_error("generate_queue: utterance " + std::to_string(u) + " ended without its final delivery");
                    return false;
                }
        }
    } else if (qst_.aborted) {   // the text callback ended a call without deliveries: the utterances that had ended keep
                                 // their frames, the others have none
        for (int k = 0; k < S_; ++k)
            if (t_.state[k] == SlotTable::ACTIVE && !release(k, false)) return false;
    }
    if (text_) {   // the error word of the rounds' descriptors (never expected: the host validated every feed)
        Q3T_HIP(hipMemcpyAsync(held_h_, e.feed_.error, 4, hipMemcpyDeviceToHost, e.stream_));
        Q3T_HIP(hipStreamSynchronize(e.stream_));
        if (held_h_[0]) {
            Q3T_HIP(hipMemsetAsync(e.feed_.error, 0, 4, e.stream_));
            set_error("generate_queue: a text feed named a row outside its buffers");
            return false;
        }
    }
    if (codes_)
        for (int u = 0; u < n_utt_; ++u)
            Q3T_HIP(hipMemcpyAsync(codes_ + (size_t)u * gp_.max_len * NCB, out_dev_ + (size_t)u * gp_.max_len * NCB,
                                   (size_t)gp_.max_len * NCB * 4, hipMemcpyDeviceToHost, e.stream_));
    Q3T_HIP(hipStreamSynchronize(e.stream_));
    if (e.persist_error()) { set_error("persistent kernel: an in-launch hand-off timed out"); fault_ = true; return false; }
    return true;
}

void Engine::QueueLoop::restore_context() {
    Engine &e = e_;
    hipStreamSynchronize(as_);
    hipStreamSynchronize(e.stream_);
    e.policy_slots_ = 0;
    std::vector<uint64_t> ident(e.max_slots_);
    for (int k = 0; k < e.max_slots_; ++k) ident[k] = (uint64_t)k;
    hipMemcpyAsync(e.utt_, ident.data(), e.max_slots_ * 8, hipMemcpyHostToDevice, e.stream_);
    hipStreamSynchronize(e.stream_);
}

bool Engine::QueueLoop::run() {
    Engine &e = e_;
    for (int u = 0; u < n_utt_; ++u) n_frames_[u] = 0;
    if (!prepare()) return false;
    // every exit drains both streams and leaves the context as generate() expects it: kernels chosen by the call's
    // own slot count, sampling keyed by slot index
    ScopeExit restore([&] { restore_context(); });
    if (!park_all()) return false;
    if (text_) {
        e.text_stats = TextStats{};
        tp_.text_vocab = e.c_.text_vocab; tp_.max_trailing = e.max_trailing_; tp_.tts_eos = e.c_.tts_eos;
        tp_.dev_hold = dev_hold_;
        tp_.begin(text_->open, n_tokens_in_, &e.feed_.round, tlog_);
        e.feed_.next = 0;
    }
    ScopeExit feed_drain([&] { if (text_) e.drain_text_rounds(); });
    if (!admit() || !activate()) return false;
    fam_ = queue_family(S_, e.mm_ok_, gemm_mfma_min_batch());
    e.policy_slots_ = S_;
    return loop() && finish();
}

// ------------------------------------------------------------------------------------------------ the open queue
// (DESIGN 2f "Arrivals")  The device side is the closed queue's with records: the same admission batches (ragged
// prefill, waiting position 10), activations, frame graphs and collections.  What differs is the host side: the
// utterances come from the arrival callback (ArrivalPlanner), live in the arrival log and are named by its handles.

// the per-utterance tables follow the log's rows
void Engine::QueueLoop::sync_tables() {
    const size_t n = alog_->e.size();
    cap_.resize(n, 0); plens_.resize(n, 0); ups_.resize(n);
    tok_eff_.resize(n, nullptr); nt_eff_.resize(n, 0); spk_eff_.resize(n, nullptr); nf_.resize(n, 0);
    qst_.delivered.resize(n, 0); qst_.stopped.resize(n, 0); qst_.finaled.resize(n, 0);
    qs_.grow(n);
    tokens_ = tok_eff_.data(); n_tokens_ = nt_eff_.data(); speaker_ = spk_eff_.data(); n_frames_ = nf_.data();
    for (int h = 0; h < (int)n; ++h)
        if (alog_->e[h].id >= 0) bind(h);
}

// handle h's rows from its log entry
void Engine::QueueLoop::bind(int h) {
    const ArrivalLog::Entry &x = alog_->e[h];
    cap_[h] = x.up.max_len; plens_[h] = x.plen; ups_[h] = x.up;
    tok_eff_[h] = x.tokens.data(); nt_eff_[h] = (int)x.tokens.size();
    spk_eff_[h] = x.speaker.empty() ? nullptr : x.speaker.data();
}

bool Engine::QueueLoop::prepare_open() {
    Engine &e = e_;
    mixed_plen_ = true;   // prompt lengths are not known ahead: free slots wait above every prompt
    plen_ = 10;
    if (gp_.max_len > e.codes_max_len_) { set_error("max_len exceeds the code buffer"); return false; }
    if (!e.alloc_admission()) return false;
    e.q_slots_ = S_;
    as_ = (S_ == 1 && e.persist_enabled()) ? e.stream_ : e.astream_;
    e.rec_on_ = S_ > 1;
    e.own_max_len_ = true;
    if (!e.set_seed(gp_.seed, e.stream_)) return false;
    if (!qs_.begin()) return false;
    if (!e.ensure_pinned(((size_t)S_ * 19 + 2) * 4)) return false;   // (the layout of prepare())
    pin_ = static_cast<int *>(e.pin_);
    done_h_ = pin_ + (size_t)S_ * 16; tgt_h_ = pin_ + (size_t)S_ * 17; park_ = pin_ + (size_t)S_ * 18;
    held_h_ = pin_ + (size_t)S_ * 18 + 2;
    for (int k = 0; k < S_; ++k) held_h_[k] = 0;
    park_[0] = 0;
    park_[1] = plen_;
    // a re-run: what ended before the fault leaves the log, every handle in limbo is free (the chunks that named it
    // died with the run), and the utterances still alive are admitted again, in id order
    sync_tables();
    retire_arrivals(*alog_, t_, qst_, qs_.run(), 0, SIZE_MAX);
    ap_.max_active = max_active_;
    ap_.hidden = e.c_.hidden;
    ap_.begin(*alog_);
    return true;
}

// at most one ask of the arrival callback (if the planner's rules allow one), then the admission of what waits
bool Engine::QueueLoop::arrivals() {
    if (!t_.batch_tgt.empty()) return true;
    std::vector<int> acc;
    bool grown = false, aborted = false;
    const std::string err = ap_.ask(t_, *alog_, qs_.pending(), arrive_, arrive_user_, &QueueLoop::check_cb, this, acc, &grown, &aborted);
    if (!err.empty()) { set_error(err); return false; }
    if (aborted) { qst_.aborted = true; return true; }
    if (grown) sync_tables();
    for (int h : acc) { bind(h); nf_[h] = 0; }
    if (!acc.empty()) f_mark_ = f_;
    return ap_.waiting.empty() || admit_open();
}

bool Engine::QueueLoop::admit_open() {   // admit() with the utterances taken from the planner's waiting list
    Engine &e = e_;
    std::vector<int> tgt, utt;
    t_.pick_waiting(ap_.waiting, max_active_, tgt, utt);
    if (tgt.empty()) return true;
    if (as_ != e.stream_) {
        Q3T_HIP(hipEventRecord(rev_, e.stream_));
        Q3T_HIP(hipStreamWaitEvent(as_, rev_, 0));
    }
    if (!e.admit_batch(tgt, utt, tokens_, n_tokens_, speaker_, ups_, plens_, true, as_, tgt_h_, batch_tl_)) return false;
    Q3T_HIP(hipEventRecord(aev_, as_));
    t_.admitted(tgt, utt, batch_tl_);
    ap_.admitted(tgt.size());
    return true;
}

// after deliveries: the utterances that had their final delivery or were cancelled leave the log and the tables
bool Engine::QueueLoop::retire() {
    for (int h = 0; h < (int)alog_->e.size(); ++h)
        if (alog_->e[h].id >= 0 && qst_.finaled[h] && !qst_.stopped[h] && qst_.delivered[h] != n_frames_[h]) {
            set_error("generate_queue_open: utterance " + std::to_string(alog_->e[h].id) + " ended without its final delivery");
            return false;
        }
    retire_arrivals(*alog_, t_, qst_, qs_.run(), qs_.collected(), qs_.delivered());
    return true;
}

bool Engine::QueueLoop::loop_open() {
    Engine &e = e_;
    int fin_seen = 0;
    while (!qst_.aborted && !ap_.finished(t_, *alog_)) {
        if (t_.n_active() == 0) {
            // nothing runs, so nothing runs behind the pending deliveries: hand them out.  Then the ask (with no slot
            // busy it is the idle one, which may block), the admission of what it brought, and the wait for the batch
            if (!deliver(INT_MAX) || !retire()) return false;
            if (qst_.aborted) break;
            if (!arrivals()) return false;
            if (qst_.aborted) break;
            if (!t_.batch_tgt.empty()) {
                Q3T_HIP(hipEventSynchronize(aev_));
                if (!activate()) return false;
                f_mark_ = f_;
                polled_ = false;
            }
            continue;
        }
        hipGraphExec_t fg = nullptr;
        if (!frame_graph(&fg)) return false;
        if (!e.persist_fault_hook(S_, (e.persist_ ? 1 : 0) + (e.persist_cp_ ? 1 : 0))) return false;
        Q3T_HIP(hipGraphLaunch(fg, e.stream_));
        ++f_;
        t_.launched();
        if (f_ % qs_.interval() == 0) {   // a tick, as in loop()
            for (int k = 0; k < S_; ++k) sel_[k] = t_.state[k] == SlotTable::ACTIVE;
            if (!qs_.collect(t_.slot_utt, sel_, false, f_ + qs_.interval())) return false;
        }
        if (!deliver(f_) || !retire()) return false;
        if (qst_.aborted) break;
        if (polled_ && !reap()) return false;
        if (t_.n_fin != fin_seen) { fin_seen = t_.n_fin; f_mark_ = f_; }
        if (!t_.batch_tgt.empty() && (as_ == e.stream_ || hipEventQuery(aev_) == hipSuccess)) {
            if (!activate()) return false;
            f_mark_ = f_;
        }
        if (!arrivals()) return false;
        if (qst_.aborted) break;
        if (as_ == e.stream_ && !t_.batch_tgt.empty()) {
            if (!activate()) return false;
            f_mark_ = f_;
        }
        if (!poll()) return false;
        if (queue_no_progress(f_ - f_mark_, t_.n_busy, gp_.max_len, plen_)) { set_error("generate_queue_open: no progress"); return false; }
    }
    return true;
}

bool Engine::QueueLoop::run_open() {
    Engine &e = e_;
    if (!prepare_open()) return false;
    ScopeExit restore([&] { restore_context(); });
    if (!park_all()) return false;
    fam_ = queue_family(S_, e.mm_ok_, gemm_mfma_min_batch());
    e.policy_slots_ = S_;
    if (!loop_open() || !finish() || !retire()) return false;
    if (!qst_.aborted && alog_->n_live != 0) { set_error("generate_queue_open: an utterance ended without its final delivery"); return false; }
    return true;
}

bool Engine::generate_queue_open(const GenParams &gp, int slots, int max_active, ArriveCb arrive, QueueCb on_batch, void *user,
                                 int interval, int32_t *n_arrived, int32_t *n_finished) {
    if (n_arrived) *n_arrived = 0;
    if (n_finished) *n_finished = 0;
    if (!arrive || !on_batch) { set_error("generate_queue_open: null callback"); return false; }
    if (interval <= 0) { set_error("generate_queue_open: the delivery interval must be > 0"); return false; }
    if (gp.max_len <= 0) { set_error("generate_queue_open: max_len must be > 0"); return false; }
    if (slots > max_slots_) { set_error("generate_queue_open: more slots than the context has"); return false; }
    const int S = slots <= 0 ? max_slots_ : slots;
    // held for the whole call, also while an idle ask blocks
    DeviceLock lk(persist_exclusive(S), device_);
    QueueState qst(0);
    ArrivalLog log;
    ScopeExit rec_off([&] { rec_on_ = false; });
    for (int run = 0;; ++run) {
        QueueLoop loop(*this, gp, S, max_active, arrive, on_batch, user, interval, qst, &log);
        const bool ok = loop.run_open();
        if (n_arrived) *n_arrived = log.next_id;
        if (n_finished) *n_finished = log.n_done;
        if (ok) return true;
        if (!loop.faulted() || run == 1) return false;
        if (!persist_recover()) return false;   // as generate_queue: the re-run admits the log's live utterances again
    }
}

bool Engine::generate_queue(int n_utt,const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                            const GenParams &gp, int32_t *codes, int *n_frames, int max_active, QueueCb on_batch, void *user,
                            int interval, const UttParams *up, const TextFeed *text) {
    for (int u = 0; u < n_utt; ++u) n_frames[u] = 0;
    if (!on_batch && !codes && n_utt > 0) { set_error("generate_queue: no codes buffer and no callback"); return false; }
    if (on_batch && interval <= 0) { set_error("generate_queue: the delivery interval must be > 0"); return false; }
    // text feeds only with an open utterance: a call without one is the queue as it was, launch for launch
    int first_open = -1;
    for (int u = n_utt - 1; text && text->open && u >= 0; --u)
        if (text->open[u]) first_open = u;
    if (text && text->held)
        for (int u = 0; u < n_utt; ++u) text->held[u] = 0;
    if (first_open < 0) text = nullptr;
    if (text && !text->cb) { set_error("utterance " + std::to_string(first_open) + ": open without a text callback"); return false; }
    if (text && interval <= 0) { set_error("generate_queue: text feeds need an interval > 0"); return false; }
    TextLog tlog;
    if (text) { tlog.ids.resize(n_utt); tlog.pieces.resize(n_utt); }
    const int S = std::min(max_slots_, std::max(n_utt, 1));
    DeviceLock lk(persist_exclusive(S), device_);
    QueueState qst(std::max(n_utt, 0));
    ScopeExit rec_off([&] { rec_on_ = false; });
    if (n_utt <= 0 || gp.max_len <= 0) return true;
    for (int run = 0;; ++run) {
        QueueLoop loop(*this, n_utt, tokens, n_tokens, speaker, gp, up, codes, n_frames, max_active, on_batch, user, interval,
                       qst, text, &tlog);
        if (loop.run()) return true;
        if (!loop.faulted() || run == 1) return false;
        // a single-slot persistent launch gave up on a hand-off: continue on the launch-per-op graphs, which are
        // bit-identical, and re-run the queue (sampling is keyed by utterance, so the re-run gives the same codes; what
        // was delivered, cancelled or finished before the fault is kept in qst and not delivered again)
        if (!persist_recover()) return false;
    }
}

}  // namespace q3t
