// The open queue's host scheduling (csrc/queue_sched.h: ArrivalPlanner, ArrivalLog, retire_arrivals, with SlotTable and
// queue_deliver.h) driven as Engine::QueueLoop::loop_open drives it, against a scripted device that knows, per utterance,
// after how many frames its done flag appears.  An admission is ready by the next iteration; the done flags are read one
// iteration late; a tick's chunk is delivered one tick late and a finish chunk one frame late.  The literal expectations
// are worked out by hand from the rules in DESIGN 2f "Arrivals".  CPU only.
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "queue_sched.h"

using namespace q3t;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

typedef std::vector<int> Ints;

struct Ask { int next_id, room, running, idle; };
struct Piece { int id, n, final; };
static bool operator==(const Ask &a, const Ask &b) { return a.next_id == b.next_id && a.room == b.room && a.running == b.running && a.idle == b.idle; }
static bool operator==(const Piece &a, const Piece &b) { return a.id == b.id && a.n == b.n && a.final == b.final; }

// the scripted device and the loop around the scheduler
struct Sim {
    // the script: what ask number i returns (how many utterances, close, abort); an utterance's done flag appears after
    // done_at(key) frames, its max_len is cap(key)
    struct Answer { int n = 0; bool close = false, abort = false; };
    std::function<Answer(int ask, int room, int idle)> answer;
    std::function<int(int key)> done_at = [](int) { return 3; };
    std::function<int(int key)> cap = [](int) { return 100; };
    std::function<uint64_t(int id)> key_of = [](int id) { return (uint64_t)id; };
    std::function<bool(int id)> cancel = [](int) { return false; };   // cancel at the utterance's first delivery
    int bad_top_k_at = -1;         // the arrival with this id carries top_k = -1
    int fault_at_chunk = -1;       // the run ends as a hand-off fault before this chunk (counted over the call) is delivered
    bool on_batch_abort_at_first = false;

    const int S, max_active, interval;
    ArrivalLog log;
    QueueState st{0};
    // the record of the call
    std::vector<Ask> asks;
    Ints deliveries_at_ask;
    std::vector<std::vector<Piece>> deliveries;
    std::vector<Ints> admitted_ids;          // per run, in admission order
    std::map<int, int> cancelled, handle_of; // the ids cancelled at a delivery; the handle an id got
    std::map<int, int> finals_run1;          // the ids finalised in the first run
    std::map<int, int> frames, finals;       // per id: frames handed out, final deliveries
    std::map<int, Ints> slot_of;             // per id: the slots it took (one per run)
    std::string error;
    size_t max_rows = 0, max_limbo = 0, max_pending = 0;
    int n_asks = 0, chunks_delivered_call = 0, f_total = 0, idle_rounds = 0;
    bool aborted = false;

    Sim(int S_, int max_active_, int interval_) : S(S_), max_active(max_active_), interval(interval_) {}

    // --- one run
    struct Chunk { bool final; int due; Ints utt, header; };
    SlotTable *t = nullptr;
    ArrivalPlanner *ap = nullptr;
    QueueRun *run = nullptr;
    std::vector<int32_t> tok_buf;

    static int ask_cb(void *user, int32_t next_id, int32_t room, int32_t running, int32_t idle, Arrival *out, int32_t *n,
                      int32_t *closed) {
        Sim &s = *static_cast<Sim *>(user);
        // the rules, checked against the table itself
        CHECK(s.t->batch_tgt.empty());               // never with an admission batch in flight
        CHECK(!s.log.closed);                        // never after the close
        CHECK(s.ap->waiting.empty());                // a re-run: only after everything logged was admitted again
        int free_slots = 0;
        for (int k = 0; k < s.S; ++k) free_slots += s.t->state[k] == SlotTable::FREE;
        CHECK(room == std::min(free_slots, s.max_active - s.t->n_busy) && room > 0);
        CHECK(running == s.t->n_busy && idle == (s.t->n_busy == 0));
        CHECK(next_id == s.log.next_id);
        s.asks.push_back(Ask{next_id, room, running, idle});
        s.deliveries_at_ask.push_back((int)s.deliveries.size());
        const Answer a = s.answer(s.n_asks++, room, idle);
        if (a.abort) return 0;
        s.tok_buf.assign(6, 7);
        for (int i = 0; i < a.n; ++i) {
            if (i >= room) break;   // (the planner's buffer has `room` entries)
            out[i].tokens = s.tok_buf.data();
            out[i].n_tokens = 6;
            out[i].key = s.key_of(next_id + i);
            out[i].up.top_k = next_id + i == s.bad_top_k_at ? -1 : 50;
        }
        *n = a.n;
        *closed = a.close;
        return 1;
    }
    static std::string check_cb(void *user, int32_t id, const Arrival &a, UttParams *up, int *plen) {
        Sim &s = *static_cast<Sim *>(user);
        if (a.up.top_k < 0) return "utterance " + std::to_string(id) + ": top_k must be >= 0";
        *up = a.up;
        up->max_len = s.cap((int)a.key);
        *plen = 9;
        return std::string();
    }

    void grow() {
        const size_t n = log.e.size();
        st.delivered.resize(n, 0); st.stopped.resize(n, 0); st.finaled.resize(n, 0);
        run->run.resize(n, 0); run->gone.resize(n, 0);
        max_rows = std::max(max_rows, n);
    }

    // false: the run ended by the scripted fault (run again), or with `error`
    bool run_once() {
        SlotTable table(S);
        ArrivalPlanner planner;
        QueueRun qrun(0);
        t = &table; ap = &planner; run = &qrun;
        planner.max_active = max_active;
        planner.hidden = 4;
        grow();
        retire_arrivals(log, table, st, qrun, 0, SIZE_MAX);
        planner.begin(log);
        admitted_ids.emplace_back();
        std::vector<Chunk> pend;
        Ints collected_dev(S, 0), done_h(S, 0), held_h(S, 0), n_frames;
        std::vector<char> sel(S, 0);
        size_t n_collected = 0, n_delivered = 0;
        int f = 0;
        bool polled = false;
        auto len_of = [&](int h) { const int key = (int)log.e[h].key; return std::min(done_at(key), log.e[h].up.max_len); };
        auto cap_vec = [&] { Ints c(log.e.size(), 0); for (size_t h = 0; h < c.size(); ++h) c[h] = log.e[h].up.max_len; return c; };
        auto collect = [&](bool final, int due) {
            Chunk c{final, due, Ints(S, -1), Ints(S, 0)};
            for (int k = 0; k < S; ++k) {
                if (!sel[k]) continue;
                const int h = table.slot_utt[k];
                c.utt[k] = h;
                c.header[k] = std::min(table.ran[k], len_of(h)) - collected_dev[k];
                collected_dev[k] += c.header[k];
            }
            pend.push_back(c);
            ++n_collected;
        };
        auto release = [&](int k) { table.released(k); };
        // QueueStreamer::deliver_due + QueueLoop::deliver + retire; false: the scripted fault
        auto deliver = [&](int due) {
            size_t n = 0;
            for (size_t i = 0; i < pend.size(); ++i) if (pend[i].due <= due) n = i + 1;
            std::vector<int> stops;
            for (size_t i = 0; i < n && !st.aborted; ++i) {
                const Chunk c = pend.front();
                pend.erase(pend.begin());
                ++n_delivered;
                if (chunks_delivered_call++ == fault_at_chunk) return false;
                std::vector<QueueEntry> ent;
                queue_plan(c.header.data(), c.utt, c.final, st, qrun, ent, stops);
                if (ent.empty()) continue;
                std::sort(ent.begin(), ent.end(), [&](const QueueEntry &a, const QueueEntry &b) { return log.e[a.utt].id < log.e[b.utt].id; });
                std::vector<int32_t> stop(ent.size(), 0);
                std::vector<Piece> d;
                for (size_t j = 0; j < ent.size(); ++j) {
                    const int id = log.e[ent[j].utt].id;
                    CHECK(id >= 0);   // a delivery never names a handle whose utterance has left the log
                    CHECK(j == 0 || id > d.back().id);
                    d.push_back(Piece{id, ent[j].n, ent[j].final});
                    // (after a fault the re-run's ticks fall elsewhere: the first piece behind the skipped frames is shorter)
                    // a delivery that is not the first and leaves the utterance unfinished has exactly `interval` frames
                    if (fault_at_chunk < 0 && frames.count(id) && frames[id] > 0 && frames[id] + ent[j].n < len_of(ent[j].utt))
                        CHECK(ent[j].n == interval);
                    if (cancel(id) && !ent[j].final) { stop[j] = 1; cancelled[id] = 1; }
                    frames[id] += ent[j].n;
                    finals[id] += ent[j].final;
                    if (ent[j].final && admitted_ids.size() == 1) finals_run1[id] = 1;
                }
                deliveries.push_back(d);
                queue_commit(ent, stop.data(), !on_batch_abort_at_first, st, qrun, stops);
            }
            for (int h : stops)
                for (int k = 0; k < S; ++k)
                    if (table.state[k] == SlotTable::ACTIVE && table.slot_utt[k] == h) release(k);
            retire_arrivals(log, table, st, qrun, n_collected, n_delivered);
            max_limbo = std::max(max_limbo, log.limbo.size());
            max_pending = std::max(max_pending, pend.size());
            return true;
        };
        auto activate = [&] {
            for (int k : table.batch_tgt) { table.activated(k); collected_dev[k] = 0; }
            table.batch_tgt.clear();
        };
        // QueueLoop::arrivals
        auto arrivals = [&]() {
            if (!table.batch_tgt.empty()) return true;
            Ints acc;
            bool grown = false, ab = false;
            error = planner.ask(table, log, !pend.empty(), ask_cb, this, check_cb, this, acc, &grown, &ab);
            if (!error.empty()) return false;
            if (ab) { st.aborted = true; return true; }
            grow();
            if (planner.waiting.empty()) return true;
            Ints tgt, utt;
            table.pick_waiting(planner.waiting, max_active, tgt, utt);
            for (size_t j = 0; j < tgt.size(); ++j) {
                admitted_ids.back().push_back(log.e[utt[j]].id);
                handle_of[log.e[utt[j]].id] = utt[j];
                slot_of[log.e[utt[j]].id].push_back(tgt[j]);
            }
            if (tgt.empty()) return true;
            table.admitted(tgt, utt, Ints(tgt.size(), 0));
            planner.admitted(tgt.size());
            return true;
        };
        int guard = 0;
        while (!st.aborted && !planner.finished(table, log)) {
            if (++guard > 4000000) { error = "the loop does not end"; return false; }
            CHECK(table.n_busy <= max_active);
            if (table.n_active() == 0) {
                ++idle_rounds;
                if (!deliver(INT_MAX)) return false;
                if (st.aborted) break;
                if (!arrivals()) return false;
                if (st.aborted) break;
                if (!table.batch_tgt.empty()) { activate(); polled = false; }
                continue;
            }
            ++f;
            ++f_total;
            table.launched();
            if (f % interval == 0) {
                for (int k = 0; k < S; ++k) sel[k] = table.state[k] == SlotTable::ACTIVE;
                collect(false, f + interval);
            }
            if (!deliver(f)) return false;
            if (st.aborted) break;
            if (polled && table.ended(done_h.data(), held_h.data(), cap_vec(), sel)) {
                collect(true, f + 1);
                for (int k = 0; k < S; ++k) if (sel[k]) release(k);
            }
            if (!table.batch_tgt.empty()) activate();
            if (!arrivals()) return false;
            if (st.aborted) break;
            for (int k = 0; k < S; ++k) {   // the device: a parked slot reads 0, a running one -1 until its flag appears
                const int h = table.slot_utt[k];
                done_h[k] = table.state[k] != SlotTable::ACTIVE ? 0 : table.ran[k] >= done_at((int)log.e[h].key) ? done_at((int)log.e[h].key) : -1;
            }
            table.polled();
            polled = true;
        }
        aborted = st.aborted;
        if (!st.aborted) {
            if (!deliver(INT_MAX)) return false;
            CHECK(log.n_live == 0);
        }
        return true;
    }
    // the call: a second run after a scripted fault
    bool call() {
        if (run_once()) return true;
        if (!error.empty()) return false;
        return run_once();
    }
};

// ---- 1. when the source is asked, with which room and idle; the loop ends at close plus drain
static void test_ask_rules() {
    // two slots, ticks every 4 frames.  Ask 0 brings utterance 0 (3 frames), ask 2 utterance 1 (2 frames), ask 3 closes
    Sim s(2, 2, 4);
    s.done_at = [](int key) { return key == 0 ? 3 : 2; };
    s.answer = [](int ask, int, int) { Sim::Answer a; a.n = ask == 0 || ask == 2; a.close = ask == 3; return a; };
    CHECK(s.call() && s.error.empty());
    // ask 0: nothing busy, idle.  asks 1, 2 (after frames 1, 2): one slot busy.  After frame 3 utterance 1 is activated and
    // both slots are busy: no room, no ask.  After frame 4 utterance 0 has left its slot: room 1 again
    CHECK(s.asks == (std::vector<Ask>{{0, 2, 0, 1}, {1, 1, 1, 0}, {1, 1, 1, 0}, {2, 1, 1, 0}}));
    // the tick after frame 4 (delivered at frame 5, behind it the finish chunk of utterance 0, which holds no new frame),
    // then the finish chunk of utterance 1
    CHECK(s.deliveries == (std::vector<std::vector<Piece>>{{{0, 3, 0}, {1, 1, 0}}, {{0, 0, 1}}, {{1, 1, 1}}}));
    CHECK(s.f_total == 6 && s.log.next_id == 2 && s.log.n_done == 2 && s.log.closed);
    CHECK(s.admitted_ids == (std::vector<Ints>{{0, 1}}) && s.slot_of[0] == (Ints{0}) && s.slot_of[1] == (Ints{1}));

    // max_active 2 of 4: never more than two busy, room never above 2 (checked at every ask), every utterance whole
    Sim m(4, 2, 4);
    m.done_at = [](int key) { return 2 + key % 5; };
    m.answer = [](int ask, int room, int) { Sim::Answer a; a.n = ask < 40 ? room : 0; a.close = ask >= 40; return a; };
    CHECK(m.call() && m.error.empty());
    for (const Ask &a : m.asks) CHECK(a.room <= 2 && a.running <= 2);
    CHECK(m.log.next_id == m.log.n_done && m.log.next_id > 10);
    for (int id = 0; id < m.log.next_id; ++id) CHECK(m.frames[id] == 2 + id % 5 && m.finals[id] == 1);

    // an utterance that stops at its max_len (its done flag never appears)
    Sim c(1, 1, 4);
    c.done_at = [](int) { return 1000; };
    c.cap = [](int) { return 6; };
    c.answer = [](int ask, int, int) { Sim::Answer a; a.n = ask == 0; a.close = true; return a; };
    CHECK(c.call() && c.frames[0] == 6 && c.finals[0] == 1);
}

// ---- 2. the queue goes empty and takes up work again; abort
static void test_empty_and_abort() {
    // one utterance, then nothing for a while: once it has drained the source is asked with idle = 1 (three times without
    // an answer: blocking is its job), then hands over one more and closes
    Sim s(2, 2, 4);
    s.answer = [](int, int, int) { return Sim::Answer(); };
    int idle_asks = 0;
    s.answer = [&](int ask, int, int idle) {
        Sim::Answer a;
        if (ask == 0) a.n = 1;
        if (ask > 0 && idle) { ++idle_asks; if (idle_asks == 4) { a.n = 1; a.close = true; } }
        return a;
    };
    CHECK(s.call() && s.error.empty());
    CHECK(idle_asks == 4 && s.log.next_id == 2 && s.log.n_done == 2);
    CHECK(s.frames[0] == 3 && s.frames[1] == 3 && s.finals[0] == 1 && s.finals[1] == 1);
    // the final delivery of utterance 0 came before the first idle ask after it: nothing waits behind a blocking ask
    CHECK(s.deliveries.size() == 4 && s.deliveries[0] == (std::vector<Piece>{{0, 3, 0}}) && s.deliveries[1] == (std::vector<Piece>{{0, 0, 1}}));
    for (size_t i = 1; i < s.asks.size(); ++i) CHECK(s.asks[i].idle == 0 || s.deliveries_at_ask[i] >= 2);
    CHECK(s.slot_of[1] == (Ints{0}));   // the freed slot is taken again

    // the arrival callback returns 0: the call ends, what ran keeps what it was handed
    Sim a(2, 2, 4);
    a.done_at = [](int) { return 50; };
    a.answer = [](int ask, int, int) { Sim::Answer r; r.n = ask == 0; r.abort = ask == 9; return r; };
    CHECK(a.call() && a.error.empty() && a.aborted);
    CHECK(a.log.next_id == 1 && a.log.n_done == 0 && a.frames[0] == 4 && a.finals[0] == 0);
    // the delivery callback returns 0: the same
    Sim b(2, 2, 4);
    b.done_at = [](int) { return 50; };
    b.on_batch_abort_at_first = true;
    b.answer = [](int ask, int, int) { Sim::Answer r; r.n = ask == 0; return r; };
    CHECK(b.call() && b.aborted && b.deliveries.size() == 1 && b.frames[0] == 4);
}

// ---- 3. the log's replay after a fault
static void test_replay() {
    // five utterances of 3, 9, 4, 9, 5 frames through 2 slots; the fault comes before the call's chunk 4
    auto script = [](Sim &s) {
        s.done_at = [](int key) { static const int d[5] = {3, 9, 4, 9, 5}; return d[key]; };
        s.answer = [](int, int room, int) { Sim::Answer a; a.n = room; return a; };
        s.answer = [&s](int, int room, int) {
            Sim::Answer a;
            a.n = std::min(room, 5 - s.log.next_id);
            a.close = s.log.next_id + a.n == 5;
            return a;
        };
    };
    Sim ref(2, 2, 4);
    script(ref);
    CHECK(ref.call() && ref.error.empty());
    static const int want[5] = {3, 9, 4, 9, 5};
    for (int id = 0; id < 5; ++id) CHECK(ref.frames[id] == want[id] && ref.finals[id] == 1);

    for (int fault_at = 0; fault_at < (int)ref.chunks_delivered_call; ++fault_at) {
        Sim s(2, 2, 4);
        script(s);
        s.fault_at_chunk = fault_at;
        CHECK(s.call() && s.error.empty());
        CHECK(s.admitted_ids.size() == 2);
        // nothing is delivered twice, nothing is lost, one final each
        for (int id = 0; id < 5; ++id) CHECK(s.frames[id] == want[id] && s.finals[id] == 1);
        CHECK(s.log.next_id == 5 && s.log.n_done == 5);
        // the re-run admits first, in id order, the utterances accepted and not finalised before the fault; the ones
        // that had their final delivery are not admitted again; the callback is asked only after them (checked in the
        // callback: nothing waits when it is asked)
        const Ints &second = s.admitted_ids[1];
        for (size_t i = 1; i < second.size(); ++i) CHECK(second[i] > second[i - 1]);
        // (not again: an utterance finalised in run 1 has finals == 1 in total, checked above, and is in no second list)
        for (int id : s.admitted_ids[0]) {
            bool again = false;
            for (int id2 : second) again = again || id2 == id;
            CHECK(again || s.finals_run1.count(id));
        }
    }
    // the literal case: fault before chunk 2.  Run 1: ask 0 brings 0 and 1.  Tick at frame 4 (chunk 0: 0 has 3 frames, 1
    // has 4), the finish chunk of 0 (chunk 1), utterance 2 takes its slot; chunk 2 is the tick of frame 8.  Utterances 1
    // and 2 both end at frame 10; with no slot busy and chunks pending the source is not asked, the chunks are handed
    // out first, and chunk 2 is the fault: 3 and 4 never arrived in run 1
    Sim s(2, 2, 4);
    script(s);
    s.fault_at_chunk = 2;
    CHECK(s.call());
    CHECK(s.admitted_ids[0] == (Ints{0, 1, 2}));
    CHECK(s.admitted_ids[1] == (Ints{1, 2, 3, 4}));   // 0 was finalised: not again; 1 and 2 before anything new
    CHECK(s.deliveries[0] == (std::vector<Piece>{{0, 3, 0}, {1, 4, 0}}) && s.deliveries[1] == (std::vector<Piece>{{0, 0, 1}}));
    // the re-run's first tick: utterance 1's first 4 frames were delivered before the fault and are skipped
    CHECK(s.deliveries[2] == (std::vector<Piece>{{2, 4, 0}}));
}

// ---- 4. bounded host state
static void test_bounded() {
    // 100,000 utterances of 1..9 frames through 4 slots, the source always fills the room; every 7th is cancelled at its
    // first delivery.  Every table has as many rows as the log; the bound is 4 S: S in slots, S that left their slot and
    // wait one frame for their final delivery, and the handles of cancelled utterances a pending chunk may still name
    // (at most S cancels per tick chunk, each waiting for at most the two chunks behind it)
    const int S = 4, N = 100000;
    Sim s(S, S, 4);
    s.done_at = [](int key) { return 1 + key % 9; };
    s.cancel = [](int id) { return id % 7 == 3; };
    s.answer = [&s](int, int room, int) {
        Sim::Answer a;
        a.n = std::min(room, N - s.log.next_id);
        a.close = s.log.next_id + a.n == N;
        return a;
    };
    CHECK(s.call() && s.error.empty());
    CHECK(s.log.next_id == N && s.log.n_done == N && s.log.n_live == 0);
    std::printf("bounded: %d arrivals, %zu table rows, limbo <= %zu, pending chunks <= %zu\n", N, s.max_rows, s.max_limbo, s.max_pending);
    CHECK(s.max_rows <= (size_t)4 * S);
    CHECK(s.log.e.size() == s.max_rows && s.st.delivered.size() == s.max_rows && s.st.finaled.size() == s.max_rows &&
          s.st.stopped.size() == s.max_rows);
    CHECK(s.log.free_h.size() + s.log.limbo.size() == s.log.e.size());
    for (const ArrivalLog::Entry &x : s.log.e) CHECK(x.id == -1 && x.tokens.capacity() == 0 && x.speaker.capacity() == 0);
    CHECK(s.max_pending <= 4);
    long long total = 0;
    for (int id = 0; id < N; ++id) {
        // (an utterance whose first delivery is its final one cannot be cancelled)
        if (s.cancelled.count(id)) { CHECK(id % 7 == 3 && s.finals[id] == 0 && s.frames[id] >= 1); }
        else { CHECK(s.frames[id] == 1 + id % 9 && s.finals[id] == 1); }
        total += s.frames[id];
    }
    CHECK(total > 4 * N && s.cancelled.size() > 1000);

    // a cancelled utterance's handle waits while a pending chunk can still name it.  Two utterances of 20 frames; 0 is
    // cancelled at its first delivery (the tick of frame 4, handed out at frame 8 when the tick of frame 8, which names
    // it too, has been collected).  Utterance 2 arrives into the freed slot at once and must not get handle 0, or the
    // four frames of utterance 0 in that pending chunk would be taken for its own
    Sim c(2, 2, 4);
    c.done_at = [](int) { return 20; };
    c.cancel = [](int id) { return id == 0; };
    c.answer = [&c](int, int room, int) {
        Sim::Answer a;
        a.n = std::min(room, 3 - c.log.next_id);
        a.close = c.log.next_id + a.n == 3;
        return a;
    };
    CHECK(c.call() && c.error.empty());
    CHECK(c.max_limbo == 1 && c.handle_of[0] == 0 && c.handle_of[1] == 1 && c.handle_of[2] == 2 && c.slot_of[2] == (Ints{0}));
    CHECK(c.frames[0] == 4 && c.finals[0] == 0 && c.frames[1] == 20 && c.frames[2] == 20 && c.finals[2] == 1);
    CHECK(c.log.n_done == 3 && c.log.free_h.size() == 3);
}

// ---- 5. rejections, with the messages the C API hands on
static void test_rejections() {
    {   // more than room
        Sim s(4, 3, 4);
        s.answer = [](int, int room, int) { Sim::Answer a; a.n = room + 1; return a; };
        CHECK(!s.call());
        CHECK(s.error == "utterance 0: the arrival callback returned 4 utterances for a room of 3");
        CHECK(s.log.next_id == 0 && s.log.n_live == 0 && s.log.e.empty());
    }
    {   // a bad record in the second answer: the call ends naming its id, nothing of that answer is accepted
        Sim s(4, 4, 4);
        s.bad_top_k_at = 3;
        s.answer = [](int, int, int) { Sim::Answer a; a.n = 2; return a; };
        CHECK(!s.call());
        CHECK(s.error == "utterance 3: top_k must be >= 0");
        CHECK(s.log.next_id == 2 && s.log.n_live == 2);
    }
    {   // a negative count
        Sim s(2, 2, 4);
        s.answer = [](int, int, int) { Sim::Answer a; a.n = -1; return a; };
        CHECK(!s.call() && s.error == "utterance 0: the arrival callback returned -1 utterances for a room of 2");
    }
    {   // the ids run out
        Sim s(2, 2, 4);
        s.log.next_id = INT32_MAX - 1;
        s.answer = [](int, int, int) { Sim::Answer a; a.n = 2; return a; };
        CHECK(!s.call() && s.error == "arrival ids exhausted: a call takes at most 2^31 - 1 utterances");
        Sim e(2, 2, 4);
        e.log.next_id = INT32_MAX;
        e.answer = [](int, int, int) { Sim::Answer a; a.n = 1; return a; };
        CHECK(!e.call() && e.error == "arrival ids exhausted: a call takes at most 2^31 - 1 utterances" && e.asks.empty());
    }
    // the stuck bound counts from the last arrival, activation or release, with the busy count
    CHECK(!queue_no_progress(3 * (24 + 10 + 2), 2, 24, 10) && queue_no_progress(3 * (24 + 10 + 2) + 1, 2, 24, 10));
}

int main() {
    test_ask_rules();
    test_empty_and_abort();
    test_replay();
    test_bounded();
    test_rejections();
    std::printf(fails ? "queue_arrivals: %d failures\n" : "queue_arrivals: ok\n", fails);
    return fails ? 1 : 0;
}
