// queue_sched.h — the host decisions of the continuous-batching queue (Engine::QueueLoop, engine_queue.cpp):
// the slot table (which utterance holds which slot, what is admitted next, which slots a frame graph covers, which
// utterances ended by the polled flags) and the text-feed planner (when an open utterance is asked, what a feed adds to
// the round, the log a fallback re-run replays, the hold / release rule, the round's blob) and, for the open queue, the
// arrival planner and log (when the arrival callback is asked, what a re-run admits again).  Header-only and free of HIP
// so tests/cpp/test_queue_sched.cpp and test_queue_arrivals.cpp drive it on the CPU against a scripted device.  A
// function that can reject input returns its message (empty: ok); the caller hands it to set_error.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "queue_deliver.h"

namespace q3t {

// one utterance's own values (q3t_utt_params): what GenParams holds for the whole call, except the seed
struct UttParams {
    int language_id = 2050;    // < 0: the nothink prompt (one row shorter)
    int max_len = 0;           // 1 .. GenParams::max_len
    float rep_penalty = 1.05f;
    float temperature = 0.9f;
    int top_k = 50;
    int force_frames = 0;
};

// an utterance's length by its done word (the index of the frame whose CB0 was EOS, < 0: none yet) and its max_len
inline int frames_of(int done, int cap) { return done >= 0 ? std::min(done, cap) : cap; }

// the smallest slot count that keeps the kernel family of an S-slot batch (matrix cores from min_batch slots,
// k_attn_seq from 16), whose per-token arithmetic every frame graph of the queue reproduces
inline int queue_family(int S, bool mm_ok, int min_batch) { return !mm_ok ? 1 : S >= 16 ? 16 : S >= min_batch ? min_batch : S; }
// frame graph over slots [0, S_eff): hi = the highest busy slot + 1, rounded up to 8, never below the family and never
// above S: a draining queue stops paying for parked slots
inline int frame_slots(int S, int fam, int hi) { return fam < S ? std::max(fam, std::min(S, (hi + 7) / 8 * 8)) : S; }
// the loop clock past which a queue that has not finished is stuck
inline bool queue_no_progress(int f, int n_utt, int max_len, int plen) { return f > (n_utt + 1) * (max_len + plen + 2); }

// Per slot: FREE (parked, waiting for an admission), PENDING (its admission batch is in flight), ACTIVE (in the frame
// loop).  ran[k]: the frames launched for slot k's utterance (while it was active and not held); ran_polled[k]: the same
// when the done flags the host now holds were copied.  Without text feeds a slot runs every frame of the loop.
struct SlotTable {
    enum { FREE, PENDING, ACTIVE };
    std::vector<int> state, slot_utt, tl;   // tl: the slot's trailing-text length, from its admission
    std::vector<int> ran, ran_polled;
    std::vector<char> hheld, fresh;         // the host holds the slot (text feeds); activated since the last asks
    std::vector<int> batch_tgt;             // the admission batch in flight (at most one)
    int next = 0, n_busy = 0, n_fin = 0;    // the next utterance to admit; slots not free; utterances that left their slot
    explicit SlotTable(int S) : state(S, FREE), slot_utt(S, -1), tl(S, 0), ran(S, 0), ran_polled(S, 0), hheld(S, 0), fresh(S, 0) {}
    int slots() const { return (int)state.size(); }

    // the next admission batch: every free slot in increasing index, utterances next, next + 1, ..., up to n_utt and to
    // max_active busy slots
    void pick_admission(int n_utt, int max_active, std::vector<int> &tgt, std::vector<int> &utt) const {
        tgt.clear(); utt.clear();
        for (int k = 0; k < slots() && next + (int)tgt.size() < n_utt && n_busy + (int)tgt.size() < max_active; ++k)
            if (state[k] == FREE) { tgt.push_back(k); utt.push_back(next + (int)tgt.size() - 1); }
    }
    // the same for the open queue: the utterances come from `waiting` (accepted arrivals not yet admitted, in id order)
    void pick_waiting(const std::vector<int> &waiting, int max_active, std::vector<int> &tgt, std::vector<int> &utt) const {
        tgt.clear(); utt.clear();
        for (int k = 0; k < slots() && tgt.size() < waiting.size() && n_busy + (int)tgt.size() < max_active; ++k)
            if (state[k] == FREE) { tgt.push_back(k); utt.push_back(waiting[tgt.size() - 1]); }
    }
    void admitted(const std::vector<int> &tgt, const std::vector<int> &utt, const std::vector<int> &batch_tl) {
        for (size_t j = 0; j < tgt.size(); ++j) {
            state[tgt[j]] = PENDING;
            slot_utt[tgt[j]] = utt[j];
            tl[tgt[j]] = batch_tl[j];
        }
        next += (int)tgt.size();
        n_busy += (int)tgt.size();
        batch_tgt = tgt;
    }
    void activated(int k) { state[k] = ACTIVE; ran[k] = 0; hheld[k] = 0; fresh[k] = 1; }
    void released(int k) { state[k] = FREE; slot_utt[k] = -1; --n_busy; ++n_fin; hheld[k] = 0; }
    int frame_slots(int fam) const {
        int hi = 0;
        for (int k = 0; k < slots(); ++k) if (state[k] != FREE) hi = k + 1;
        return q3t::frame_slots(slots(), fam, hi);
    }
    void launched() { for (int k = 0; k < slots(); ++k) ran[k] += state[k] == ACTIVE && !hheld[k]; }
    void polled() { ran_polled = ran; }
    int n_active() const { int n = 0; for (int k = 0; k < slots(); ++k) n += state[k] == ACTIVE; return n; }
    int n_run() const { int n = 0; for (int k = 0; k < slots(); ++k) n += state[k] == ACTIVE && !hheld[k]; return n; }
    // the slots whose utterance ended by the polled flags (done_h / held_h, copied when slot k had run ran_polled[k]
    // frames; max_len: per utterance): a held slot's done flag is its hold, not an end (its done word becomes -1), and
    // a slot the host holds may have ended before the hold ran (its real EOS stays and it is not flagged held).
    // True if any slot is selected
    bool ended(int *done_h, const int *held_h, const std::vector<int> &max_len, std::vector<char> &sel) const {
        bool any = false;
        for (int k = 0; k < slots(); ++k) {
            if (held_h[k]) done_h[k] = -1;
            sel[k] = state[k] == ACTIVE && !(done_h[k] < 0 && ran_polled[k] < max_len[slot_utt[k]]);
            any = any || sel[k];
        }
        return any;
    }
};

// what the open utterances of a queue were fed (text feeds), kept across a fallback re-run: the re-run replays it
// against the same `frames` schedule instead of asking the callback again
struct TextLog {
    struct Piece { int frames, n; bool end; };
    std::vector<std::vector<int32_t>> ids;     // per utterance, every fed id
    std::vector<std::vector<Piece>> pieces;    // per utterance: at `frames` generated frames, n ids (and the end)
};

// A round: what the asks of one loop iteration produced.  New text ids of some slots (ids, with one trailing tts_eos id
// if an utterance closed), where their projected rows go (rows: source index, slot, trailing row), the counters they
// publish (commit: slot, trailing_len, n_tokens) and the slots to hold / release (hold / rel, [S] masks).
struct TextRound {
    std::vector<int> ids, rows, commit, hold, rel;
    bool any_hold = false, any_rel = false;
    void reserve(int cap_rows, int S) {
        ids.reserve(cap_rows); rows.reserve((size_t)3 * cap_rows); commit.reserve((size_t)3 * S);
        hold.reserve(S); rel.reserve(S);
    }
    bool empty() const { return ids.empty() && commit.empty() && !any_hold && !any_rel; }
    struct Layout { size_t o_rel, o_commit, o_rows, o_ids; int n_ids, n_rows, n_commit; size_t ints; };
    // the blob [hold S | release S | commit 3 S, zero-padded | rows 3 n | ids n]
    Layout pack(int *blob, int S) const {
        Layout l;
        l.n_ids = (int)ids.size(); l.n_rows = (int)rows.size() / 3; l.n_commit = (int)commit.size() / 3;
        l.o_rel = S; l.o_commit = (size_t)2 * S; l.o_rows = (size_t)5 * S; l.o_ids = l.o_rows + (size_t)3 * l.n_rows;
        l.ints = l.o_ids + l.n_ids;
        std::copy(hold.begin(), hold.end(), blob);
        std::copy(rel.begin(), rel.end(), blob + l.o_rel);
        std::fill(blob + l.o_commit, blob + l.o_rows, 0);
        std::copy(commit.begin(), commit.end(), blob + l.o_commit);
        std::copy(rows.begin(), rows.end(), blob + l.o_rows);
        std::copy(ids.begin(), ids.end(), blob + l.o_ids);
        return l;
    }
};

// An open utterance (text feeds): its head [3 role ids, >= 1 text id] runs as the head || five tts_pad ids, whose rows
// are exactly the head's (the five are dropped when the prompt rows are planned)
inline std::string open_head(int u, const int32_t *ids, int n, int text_vocab, int max_trailing, int tts_pad,
                             std::vector<int32_t> &padded) {
    const std::string who = "utterance " + std::to_string(u) + ": ";
    if (n < 4) return who + "an open utterance needs a head of at least 4 ids";
    if (n - 4 + 1 > max_trailing) return who + "head too long for the trailing-text buffer";
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= text_vocab) return who + "text token out of range";
    padded.assign(ids, ids + n);
    padded.insert(padded.end(), 5, tts_pad);
    return std::string();
}

// Text feeds: per utterance the known trailing rows K (rows_known) and whether its text has ended.  An open utterance
// that holds a slot is asked when it was activated (before its first frame), at every tick, and on every iteration on
// which it has no row for its next frame.  Each answer is validated, logged (a fallback re-run replays the log instead
// of asking) and added to the round; then every open slot is held or released by `frames >= K && !closed`.
// n_tokens is published as K + 9 with every feed, so CB0's EOS ramp (expected = max(20, 4 * n_tokens)) sees a count
// that grows.  That never changes a selection: while the text is open the slot only runs frames f < K, and the
// selection at the end of frame f uses frame = f + 1 <= K < 4 * (K + 9) <= 4 * (K_final + 9), so the ramp is off under
// the running count and under the final one alike; after the close the two are equal.
struct TextPlanner {
    // the text callback (Engine::TextCb): 0 ends the call
    typedef int (*AskFn)(void *user, int32_t utt, int32_t frames, int32_t rows_ahead, const int32_t **ids, int32_t *n_ids,
                         int32_t *end);
    int text_vocab = 0, max_trailing = 0, tts_eos = 0;
    // a one-slot queue holds by not launching: device masks only for slots that share a frame graph with running ones
    bool dev_hold = false;
    bool tick = false;                      // the last launch completed a tick: every open slot is asked
    std::vector<int> rows_known, replay_piece, replay_id;
    std::vector<char> is_open, closed;      // per utterance (all closed without text feeds)
    TextRound *r = nullptr;                 // the round under construction (the context's, reserved once)
    TextLog *log = nullptr;

    explicit TextPlanner(int n_utt) : is_open(n_utt, 0), closed(n_utt, 1) {}
    // open[u] != 0: utterance u is fed its text; n_head[u]: the ids of its head as the caller gave it
    void begin(const uint8_t *open, const int *n_head, TextRound *round, TextLog *tlog) {
        const int n_utt = (int)is_open.size();
        rows_known.assign(n_utt, 0); replay_piece.assign(n_utt, 0); replay_id.assign(n_utt, 0);
        for (int u = 0; u < n_utt; ++u) {
            is_open[u] = open[u] != 0;
            closed[u] = !is_open[u];
            rows_known[u] = n_head[u] - 4;
        }
        r = round;
        log = tlog;
    }
    // a piece of n ids (and the end) for utterance u in slot k: row triplets, the tts_eos placeholder (source row -1,
    // fixed up when the round is closed) and the commit (k, K + end, K + 9)
    std::string feed_piece(int u, int k, const int32_t *ids, int n, bool end) {
        const char *bad = nullptr;
        if (n < 0 || (n > 0 && !ids)) bad = "bad text feed";
        for (int i = 0; !bad && i < n; ++i)
            if (ids[i] < 0 || ids[i] >= text_vocab) bad = "fed text token out of range";
        if (!bad && rows_known[u] + n + 1 > max_trailing) bad = "text feed exceeds the trailing-text buffer";
        if (bad) return "utterance " + std::to_string(u) + ": " + bad;
        for (int i = 0; i < n; ++i) {
            r->rows.push_back((int)r->ids.size()); r->rows.push_back(k); r->rows.push_back(rows_known[u] + i);
            r->ids.push_back(ids[i]);
        }
        rows_known[u] += n;
        if (end) {   // row K becomes the tts_eos row
            closed[u] = 1;
            r->rows.push_back(-1); r->rows.push_back(k); r->rows.push_back(rows_known[u]);
        }
        if (n > 0 || end) {
            r->commit.push_back(k); r->commit.push_back(rows_known[u] + (end ? 1 : 0)); r->commit.push_back(rows_known[u] + 9);
        }
        return std::string();
    }
    // a new round: the asks of this iteration.  A slot whose log still has pieces is given the ones due by now
    // (pieces[i].frames <= ran) and is not asked.  *aborted: the callback returned 0 (the round is dropped)
    std::string ask(SlotTable &t, AskFn cb, void *user, bool *aborted) {
        const int S = t.slots();
        r->ids.clear(); r->rows.clear(); r->commit.clear();
        r->hold.assign(S, 0); r->rel.assign(S, 0);
        r->any_hold = r->any_rel = false;
        *aborted = false;
        for (int k = 0; k < S && !*aborted; ++k) {
            const int u = t.slot_utt[k];
            if (t.state[k] != SlotTable::ACTIVE || !is_open[u] || closed[u]) { t.fresh[k] = 0; continue; }
            if (!(t.fresh[k] || tick || t.ran[k] >= rows_known[u])) continue;
            t.fresh[k] = 0;
            std::vector<TextLog::Piece> &pieces = log->pieces[u];
            bool replayed = false;
            while (replay_piece[u] < (int)pieces.size() && pieces[replay_piece[u]].frames <= t.ran[k] && !closed[u]) {
                const TextLog::Piece pc = pieces[replay_piece[u]++];
                std::string err = feed_piece(u, k, log->ids[u].data() + replay_id[u], pc.n, pc.end);
                if (!err.empty()) return err;
                replay_id[u] += pc.n;
                replayed = true;
            }
            if (replayed || replay_piece[u] < (int)pieces.size()) continue;
            const int32_t *ids = nullptr;
            int32_t n = 0, end = 0;
            if (!cb(user, u, t.ran[k], std::max(0, rows_known[u] - t.ran[k]), &ids, &n, &end)) { *aborted = true; break; }
            if (n == 0 && !end) continue;
            std::string err = feed_piece(u, k, ids, n, end != 0);
            if (!err.empty()) return err;
            if (n > 0) log->ids[u].insert(log->ids[u].end(), ids, ids + n);
            pieces.push_back(TextLog::Piece{t.ran[k], n, end != 0});
            replay_piece[u] = (int)pieces.size();
            replay_id[u] = (int)log->ids[u].size();
        }
        tick = false;
        return std::string();
    }
    // the round is closed: the placeholder rows read the one trailing tts_eos id, and every open slot is held or
    // released (max_len: per utterance; held: per utterance, bumped once per transition into hold, may be null)
    void close_round(SlotTable &t, const std::vector<int> &max_len, int32_t *held) {
        bool any_eos = false;
        for (size_t i = 0; i < r->rows.size(); i += 3)
            if (r->rows[i] < 0) { r->rows[i] = (int)r->ids.size(); any_eos = true; }
        if (any_eos) r->ids.push_back(tts_eos);
        for (int k = 0; k < t.slots(); ++k) {
            const int u = t.slot_utt[k];
            if (t.state[k] != SlotTable::ACTIVE || !is_open[u]) continue;
            const bool want = !closed[u] && t.ran[k] >= rows_known[u] && t.ran[k] < max_len[u];
            if (want && !t.hheld[k]) {
                if (held) ++held[u];
                if (dev_hold) { r->hold[k] = 1; r->any_hold = true; }
            } else if (!want && t.hheld[k] && dev_hold) {
                r->rel[k] = 1; r->any_rel = true;
            }
            t.hheld[k] = want;
        }
    }
};

// ------------------------------------------------------------------------------------------------------ arrivals
// The open queue (Engine::generate_queue_open; DESIGN 2f "Arrivals"): the utterances are not known up front, they come
// from an arrival callback while the loop runs.  An accepted utterance has an id (arrival order, from 0 per call) and,
// while it lives, a handle: the index of its row in every per-utterance table of the loop (SlotTable::slot_utt,
// QueueState, QueueRun, the log below).  Handles are reused, so the tables are as large as the most utterances that
// were ever alive at once, which the slot count bounds, not as the number of arrivals so far.

// what the arrival callback hands over: read before the callback returns
struct Arrival {
    const int32_t *tokens = nullptr;
    int n_tokens = 0;
    const float *speaker = nullptr;   // hidden floats or null
    UttParams up;
    uint64_t key = 0;                 // the utterance's sampling key
};

// Every accepted arrival, copied when the callback returned and kept until its final delivery or its cancel (end()):
// what a re-run after a hand-off fault admits again, and where the admissions read the prompts from.  It also keeps
// what must survive a re-run: the next id and the close.
struct ArrivalLog {
    struct Entry {
        int32_t id = -1;              // -1: the handle is free (or in limbo)
        uint64_t key = 0;
        std::vector<int32_t> tokens;
        std::vector<float> speaker;   // empty: none
        UttParams up;                 // validated, max_len resolved
        int plen = 0;                 // its prompt rows
    };
    struct Limbo { int h; size_t stamp; };
    std::vector<Entry> e;             // by handle
    std::vector<int> free_h;
    // an ended utterance's handle is reused only when every chunk collected before it ended has been delivered: such a
    // chunk may still name the handle (a tick's chunk is delivered one tick late)
    std::vector<Limbo> limbo;
    int32_t next_id = 0, n_done = 0;  // ids handed out; utterances ended (final delivery or cancel)
    int n_live = 0;
    bool closed = false;

    // a handle for a new utterance (the tables grow by one row when none is free); *grown: e.size() changed
    int take(bool *grown) {
        *grown = free_h.empty();
        if (*grown) { e.emplace_back(); free_h.push_back((int)e.size() - 1); }
        const int h = free_h.back();
        free_h.pop_back();
        ++n_live;
        return h;
    }
    // the utterance of handle h had its final delivery or was cancelled; stamp: the chunks collected so far
    void end(int h, size_t stamp) {
        Entry &x = e[h];
        x.id = -1;
        std::vector<int32_t>().swap(x.tokens);
        std::vector<float>().swap(x.speaker);
        limbo.push_back(Limbo{h, stamp});
        --n_live;
        ++n_done;
    }
    // `delivered` chunks have been delivered: the handles in limbo that no pending chunk can name are free again
    // (reset(h): clear the handle's rows in the other tables)
    template <class F> void recycle(size_t delivered, F &&reset) {
        size_t keep = 0;
        for (const Limbo &l : limbo) {
            if (l.stamp <= delivered) { reset(l.h); free_h.push_back(l.h); }
            else limbo[keep++] = l;
        }
        limbo.resize(keep);
    }
    // the handles of the live utterances in id order: what a re-run admits again
    std::vector<int> unfinished() const {
        std::vector<int> v;
        for (int h = 0; h < (int)e.size(); ++h) if (e[h].id >= 0) v.push_back(h);
        std::sort(v.begin(), v.end(), [this](int a, int b) { return e[a].id < e[b].id; });
        return v;
    }
};

// When the arrival callback is asked, and what its answer does.  It is asked at most once per loop iteration, between
// two frames, and only when no admission batch is in flight, the source is not closed, nothing accepted is still
// waiting for a slot and room = min(free slots, max_active - busy) > 0.  idle = 1 exactly when no slot is busy (and so
// nothing runs or is pending): then the callback may block; with idle = 0 it must return at once.  It returns at most
// `room` utterances: the engine keeps no backlog.  Every arrival of an answer is validated before any is accepted.
// While deliveries are pending the idle ask waits (the loop hands them out first): nothing waits behind a blocking ask.
struct ArrivalPlanner {
    // the arrival callback (Engine::ArriveCb): 0 ends the call
    typedef int (*AskFn)(void *user, int32_t next_id, int32_t room, int32_t running, int32_t idle, Arrival *out, int32_t *n,
                         int32_t *closed);
    // the checks of an arrival (Engine::check_arrival): its message or empty; *up: the record with max_len resolved
    typedef std::string (*CheckFn)(void *ctx, int32_t id, const Arrival &a, UttParams *up, int *plen);
    int max_active = 0;               // <= the slot count
    int hidden = 0;                   // floats of a speaker row
    std::vector<int> waiting;         // handles accepted and not yet admitted, in id order
    std::vector<Arrival> buf;
    int last_room = 0, last_idle = 0; // of the last ask

    // a run begins: a re-run admits the log's unfinished utterances again, in id order, before the callback is asked
    void begin(const ArrivalLog &log) { waiting = log.unfinished(); }
    int room(const SlotTable &t) const { return std::min(t.slots(), max_active) - t.n_busy - (int)waiting.size(); }
    bool may_ask(const SlotTable &t, const ArrivalLog &log) const {
        return t.batch_tgt.empty() && !log.closed && waiting.empty() && room(t) > 0;
    }
    // the source is closed and every accepted utterance has left its slot
    bool finished(const SlotTable &t, const ArrivalLog &log) const { return log.closed && waiting.empty() && t.n_busy == 0; }
    void admitted(size_t n) { waiting.erase(waiting.begin(), waiting.begin() + n); }
    // one ask, if the rules allow it.  accepted: the handles of the utterances it brought (also in `waiting`);
    // *grown: the log has more rows than before; *aborted: the callback returned 0.  deliveries_pending: collected chunks
    // wait for their delivery
    std::string ask(const SlotTable &t, ArrivalLog &log, bool deliveries_pending, AskFn cb, void *user, CheckFn check,
                    void *cctx, std::vector<int> &accepted, bool *grown, bool *aborted) {
        accepted.clear();
        *grown = *aborted = false;
        if (!may_ask(t, log) || (t.n_busy == 0 && deliveries_pending)) return std::string();
        if (log.next_id == INT32_MAX) return "arrival ids exhausted: a call takes at most 2^31 - 1 utterances";
        const int rm = room(t);
        buf.assign(rm, Arrival());
        int32_t n = 0, cl = 0;
        last_room = rm;
        last_idle = t.n_busy == 0;
        if (!cb(user, log.next_id, rm, t.n_busy, last_idle, buf.data(), &n, &cl)) { *aborted = true; return std::string(); }
        if (n < 0 || n > rm)
            return "utterance " + std::to_string(log.next_id) + ": the arrival callback returned " + std::to_string(n) +
                   " utterances for a room of " + std::to_string(rm);
        if (n > INT32_MAX - log.next_id) return "arrival ids exhausted: a call takes at most 2^31 - 1 utterances";
        std::vector<UttParams> ups(n);
        std::vector<int> plens(n);
        for (int i = 0; i < n; ++i) {
            const std::string err = check(cctx, log.next_id + i, buf[i], &ups[i], &plens[i]);
            if (!err.empty()) return err;
        }
        for (int i = 0; i < n; ++i) {
            bool g = false;
            const int h = log.take(&g);
            *grown = *grown || g;
            ArrivalLog::Entry &x = log.e[h];
            x.id = log.next_id++;
            x.key = buf[i].key;
            x.tokens.assign(buf[i].tokens, buf[i].tokens + buf[i].n_tokens);
            if (buf[i].speaker) x.speaker.assign(buf[i].speaker, buf[i].speaker + hidden);
            else x.speaker.clear();
            x.up = ups[i];
            x.plen = plens[i];
            waiting.push_back(h);
            accepted.push_back(h);
        }
        if (cl) log.closed = true;
        return std::string();
    }
};

// After deliveries (and after the slots of cancelled utterances were released): the utterances that had their final
// delivery or were cancelled leave the log, and the handles no pending chunk can name any more are cleared for reuse.
// collected / delivered: the chunks collected / delivered so far in this run
inline void retire_arrivals(ArrivalLog &log, const SlotTable &t, QueueState &st, QueueRun &r, size_t collected, size_t delivered) {
    for (int h = 0; h < (int)log.e.size(); ++h) {
        if (log.e[h].id < 0 || !(st.finaled[h] || st.stopped[h])) continue;
        bool in_slot = false;
        for (int k = 0; k < t.slots() && !in_slot; ++k) in_slot = t.state[k] != SlotTable::FREE && t.slot_utt[k] == h;
        // (a final chunk is the last one collected that names its utterance, and chunks are delivered in order: only a
        // cancelled utterance can still be named by a pending chunk)
        if (!in_slot) log.end(h, st.stopped[h] ? collected : 0);
    }
    log.recycle(delivered, [&](int h) {
        st.delivered[h] = 0; st.stopped[h] = 0; st.finaled[h] = 0;
        r.run[h] = 0; r.gone[h] = 0;
    });
}

}  // namespace q3t
