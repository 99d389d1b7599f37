// The queue's host scheduling (csrc/queue_sched.h: SlotTable, TextPlanner, TextRound) driven as Engine::QueueLoop drives
// it, against a scripted device that knows, per utterance, after how many frames its done flag appears.  Expected values
// are literals worked out by hand from the rules in DESIGN 2f, not recomputed with the code under test.  CPU only.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "queue_sched.h"

using namespace q3t;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

typedef std::vector<int> Ints;

// ---- 1. admission and reap: the loop of QueueLoop::loop without text feeds or deliveries.  An admission is ready by the
// next iteration; the done flags are copied behind each launch and read one iteration later
static void test_admission_and_reap() {
    const int S = 3, n_utt = 7, max_active = 2;
    const int done_at[n_utt] = {3, 1, 5, 2, 9, 1, 4};
    const Ints cap(n_utt, 8);
    SlotTable t(S);
    Ints n_frames(n_utt, -1), parked(n_utt, -1), admitted_slot, admitted_utt, done_h(S, 0), held_h(S, 0);
    std::vector<char> sel(S, 0), owned(S, 0);
    auto admit = [&] {
        Ints tgt, utt;
        t.pick_admission(n_utt, max_active, tgt, utt);
        if (tgt.empty()) return;
        for (size_t j = 0; j < tgt.size(); ++j) {
            CHECK(!owned[tgt[j]]);   // no slot is handed on before released()
            owned[tgt[j]] = 1;
            admitted_slot.push_back(tgt[j]);
            admitted_utt.push_back(utt[j]);
        }
        t.admitted(tgt, utt, Ints(tgt.size(), 0));
    };
    auto activate = [&] {
        for (int k : t.batch_tgt) t.activated(k);
        t.batch_tgt.clear();
    };
    admit();
    activate();
    int f = 0;
    bool polled = false;
    while (t.n_fin < n_utt && f < 1000) {
        CHECK(t.n_busy <= max_active);
        if (t.n_active() == 0) { if (t.batch_tgt.empty()) admit(); activate(); polled = false; continue; }
        ++f;
        t.launched();
        if (polled && t.ended(done_h.data(), held_h.data(), cap, sel))
            for (int k = 0; k < S; ++k) {
                if (!sel[k]) continue;
                const int u = t.slot_utt[k];
                CHECK(n_frames[u] == -1);
                n_frames[u] = frames_of(done_h[k], cap[u]);
                parked[u] = done_h[k] < 0;
                t.released(k);
                owned[k] = 0;
            }
        if (!t.batch_tgt.empty()) activate();
        if (t.batch_tgt.empty() && t.next < n_utt) admit();
        for (int k = 0; k < S; ++k) {   // the device: a parked slot reads 0, a running one -1 until its flag appears
            const int u = t.slot_utt[k];
            done_h[k] = t.state[k] != SlotTable::ACTIVE ? 0 : t.ran[k] >= done_at[u] ? done_at[u] : -1;
        }
        t.polled();
        polled = true;
    }
    CHECK(admitted_utt == (Ints{0, 1, 2, 3, 4, 5, 6}));    // each once, in index order
    CHECK(admitted_slot == (Ints{0, 1, 1, 0, 0, 1, 1}));   // the lowest free slot; two busy slots never reach slot 2
    CHECK(n_frames == (Ints{3, 1, 5, 2, 8, 1, 4}));        // min(done, cap)
    CHECK(parked == (Ints{0, 0, 0, 0, 1, 0, 0}));          // only the one stopped at its max_len is still running
    CHECK(f == 18 && t.n_fin == 7 && t.n_busy == 0 && t.next == 7);

    // "held is not ended": a held flag beside a done word >= 0 is the hold; a slot the host holds whose flag is clear
    // ended before the hold ran
    SlotTable h(2);
    h.admitted(Ints{0, 1}, Ints{0, 1}, Ints{0, 0});
    h.activated(0); h.activated(1);
    h.ran = Ints{5, 3};
    h.hheld[0] = h.hheld[1] = 1;
    h.polled();
    Ints dh = {5, 3}, hh = {1, 0};
    std::vector<char> s2(2, 0);
    CHECK(h.ended(dh.data(), hh.data(), Ints{8, 8}, s2));
    CHECK(!s2[0] && s2[1] && dh[0] == -1 && dh[1] == 3);
    CHECK(h.n_active() == 2 && h.n_run() == 0);
    h.launched();   // held slots gain no frame
    CHECK(h.ran == (Ints{5, 3}));
    // a PENDING slot is never selected, whatever its (parked) done word says
    SlotTable p(1);
    p.admitted(Ints{0}, Ints{0}, Ints{0});
    Ints dp = {0}, hp = {0};
    std::vector<char> s1(1, 1);
    CHECK(!p.ended(dp.data(), hp.data(), Ints{8}, s1) && !s1[0]);
    // the no-progress bound: f > (n_utt + 1) * (max_len + plen + 2)
    CHECK(!queue_no_progress(160, 7, 8, 10) && queue_no_progress(161, 7, 8, 10));
}

// ---- 2. the frame graph's slot count
static void test_frame_slots() {
    const int cases[][4] = {{64, 16, 1, 16}, {64, 16, 16, 16}, {64, 16, 17, 24}, {64, 16, 57, 64}, {12, 4, 3, 8}, {12, 4, 9, 12},
                            {8, 4, 0, 4},    {4, 4, 2, 4},     {3, 3, 1, 3},     {24, 1, 5, 8},    {24, 1, 0, 1}};
    for (const auto &c : cases) {
        CHECK(frame_slots(c[0], c[1], c[2]) == c[3]);
        SlotTable t(c[0]);   // the same through the table: hi = the highest slot that is not free, + 1
        if (c[2] > 0) t.state[c[2] - 1] = SlotTable::PENDING;
        if (c[2] > 1) t.state[0] = SlotTable::ACTIVE;
        CHECK(t.frame_slots(c[1]) == c[3]);
    }
    const int fam_on[][2] = {{1, 1}, {3, 3}, {4, 4}, {15, 4}, {16, 16}, {64, 16}};
    for (const auto &c : fam_on) {
        CHECK(queue_family(c[0], true, 4) == c[1]);
        CHECK(queue_family(c[0], false, 4) == 1);
    }
}

// ---- a scripted text source: answer[(utt, frames)] = ids and the end; every call is recorded
struct Source {
    struct Answer { int utt, frames; Ints ids; bool end; };
    std::vector<Answer> answers;
    std::vector<std::pair<int, int>> calls;   // (utt, frames)
    Ints rows_ahead;
    std::vector<int32_t> buf;
    bool forbidden = false;
    static int ask(void *user, int32_t utt, int32_t frames, int32_t ahead, const int32_t **ids, int32_t *n, int32_t *end) {
        Source &s = *static_cast<Source *>(user);
        if (s.forbidden) { std::printf("FAIL: the callback was asked (utt %d, frames %d)\n", utt, frames); ++fails; }
        s.calls.push_back({utt, frames});
        s.rows_ahead.push_back(ahead);
        for (const Answer &a : s.answers)
            if (a.utt == utt && a.frames == frames) {
                s.buf.assign(a.ids.begin(), a.ids.end());
                *ids = s.buf.data(); *n = (int32_t)s.buf.size(); *end = a.end;
                return 1;
            }
        *n = 0; *end = 0;
        return 1;
    }
};

static const int TEXT_VOCAB = 152000, TTS_EOS = 151673, MAX_TRAILING = 64;

struct Feeds {   // a planner over a table whose slot k runs utterance k, every slot active
    SlotTable t;
    TextPlanner tp;
    TextRound round;
    Ints max_len;
    std::vector<int32_t> held;
    Feeds(int S, const std::vector<uint8_t> &open, const Ints &n_head, const Ints &max_len_, TextLog *log)
        : t(S), tp(S), max_len(max_len_), held(S, 0) {
        Ints all(S);
        for (int k = 0; k < S; ++k) all[k] = k;
        t.admitted(all, all, Ints(S, 0));
        for (int k = 0; k < S; ++k) t.activated(k);
        t.batch_tgt.clear();
        round.reserve(S * MAX_TRAILING + 1, S);
        tp.text_vocab = TEXT_VOCAB; tp.max_trailing = MAX_TRAILING; tp.tts_eos = TTS_EOS;
        tp.dev_hold = S > 1;
        tp.begin(open.data(), n_head.data(), &round, log);
    }
    // one loop iteration's round; the packed blob
    Ints do_round(Source &src) {
        bool aborted = false;
        const std::string err = tp.ask(t, Source::ask, &src, &aborted);
        CHECK(err.empty() && !aborted);
        tp.close_round(t, max_len, held.data());
        Ints blob(5 * t.slots() + 4 * (t.slots() * MAX_TRAILING + 1), -7);
        const TextRound::Layout l = round.pack(blob.data(), t.slots());
        blob.resize(l.ints);
        return blob;
    }
};

// ---- 3. a round's layout and the hold rule
static void test_text_round() {
    TextLog log;
    log.ids.resize(3); log.pieces.resize(3);
    // utterance 0: head of 5 ids (K = 1), fed 2 ids; utterance 1 is not open; utterance 2: head of 6 (K = 2), 1 id and the end
    Feeds F(3, {1, 0, 1}, Ints{5, 20, 6}, Ints{100, 100, 100}, &log);
    Source src;
    src.answers = {{0, 0, {100, 101}, false}, {2, 0, {200}, true}};
    const Ints blob = F.do_round(src);
    CHECK(blob == (Ints{0, 0, 0,                                   // hold
                        0, 0, 0,                                   // release
                        0, 3, 12, 2, 4, 12, 0, 0, 0,               // commit (slot, K [+ 1 at the end], K + 9), zero-padded
                        0, 0, 1, 1, 0, 2, 2, 2, 2, 3, 2, 3,        // rows (source, slot, trailing row); the eos row reads id 3
                        100, 101, 200, TTS_EOS}));
    Ints again(31);
    const TextRound::Layout l = F.round.pack(again.data(), 3);
    CHECK(again == blob);
    CHECK(l.o_rel == 3 && l.o_commit == 6 && l.o_rows == 15 && l.o_ids == 27 && l.ints == 31);
    CHECK(l.n_ids == 4 && l.n_rows == 4 && l.n_commit == 2);
    CHECK(src.calls == (std::vector<std::pair<int, int>>{{0, 0}, {2, 0}}) && src.rows_ahead == (Ints{1, 2}));
    CHECK(F.tp.rows_known == (Ints{3, 16, 3}) && F.tp.closed[2] && !F.tp.closed[0] && F.tp.closed[1]);
    CHECK(!F.round.any_hold && !F.round.any_rel && !F.round.empty());

    // the hold rule, S = 2 (device masks): slot 0 runs an open utterance with K = 1, slot 1 a closed one
    for (int S = 2; S >= 1; --S) {
        TextLog lg;
        lg.ids.resize(S); lg.pieces.resize(S);
        Feeds H(S, S == 2 ? std::vector<uint8_t>{1, 0} : std::vector<uint8_t>{1}, Ints(S, 5), Ints(S, 100), &lg);
        Source s;
        s.answers = {{0, 1, {7}, false}, {0, 2, {}, true}};
        auto masks = [&](int hold0, int rel0) {
            return H.round.hold[0] == hold0 && H.round.rel[0] == rel0 && H.round.any_hold == (hold0 != 0) &&
                   H.round.any_rel == (rel0 != 0);
        };
        const int dev = S > 1;   // a one-slot queue holds by not launching: no mask is ever set
        H.do_round(s);                               // fresh, ran 0 < K: asked, nothing comes, no hold
        CHECK(masks(0, 0) && !H.t.hheld[0] && H.held[0] == 0 && H.round.empty());
        H.t.launched();                              // ran 1
        s.answers[0].frames = -1;                    // (the source withholds its text for two rounds)
        H.do_round(s);                               // ran == K: hold
        CHECK(masks(dev, 0) && H.t.hheld[0] && H.held[0] == 1 && H.round.empty() == !dev);
        H.t.launched();                              // a held slot gains no frame
        CHECK(H.t.ran[0] == 1);
        H.do_round(s);                               // still held: no new mask, no new count
        CHECK(masks(0, 0) && H.t.hheld[0] && H.held[0] == 1 && H.round.empty());
        s.answers[0].frames = 1;
        H.do_round(s);                               // one id arrives: K = 2, release
        CHECK(masks(0, dev) && !H.t.hheld[0] && H.held[0] == 1 && !H.round.empty());
        H.t.launched();                              // ran 2
        s.answers[1].frames = -1;
        H.do_round(s);                               // ran == K again: a second transition into hold
        CHECK(masks(dev, 0) && H.t.hheld[0] && H.held[0] == 2);
        s.answers[1].frames = 2;
        H.do_round(s);                               // the end arrives: released, the tts_eos row at K = 2
        CHECK(masks(0, dev) && !H.t.hheld[0] && H.held[0] == 2 && H.tp.closed[0]);
        CHECK(H.round.ids == (Ints{TTS_EOS}) && H.round.rows == (Ints{0, 0, 2}) && H.round.commit == (Ints{0, 3, 11}));
        const size_t asked = s.calls.size();
        CHECK(asked == 6);
        for (int i = 0; i < 3; ++i) { H.t.launched(); H.do_round(s); }   // closed: never held, never asked again
        CHECK(masks(0, 0) && !H.t.hheld[0] && H.held[0] == 2 && s.calls.size() == asked && H.t.ran[0] == 5);
        if (S == 2) CHECK(H.held[1] == 0 && H.t.ran[1] == 6);   // the closed neighbour ran every frame
    }
    // no hold at ran == max_len: the slot is about to be reaped
    TextLog lg;
    lg.ids.resize(2); lg.pieces.resize(2);
    Feeds M(2, {1, 0}, Ints{6, 5}, Ints{2, 100}, &lg);
    Source s;
    M.do_round(s);
    M.t.launched(); M.t.launched();   // ran 2 == K == max_len
    M.do_round(s);
    CHECK(!M.t.hheld[0] && M.held[0] == 0 && !M.round.any_hold);
    CHECK(s.calls == (std::vector<std::pair<int, int>>{{0, 0}, {0, 2}}));
}

// ---- 4. the log and its replay
static std::vector<Ints> run_schedule(Feeds &F, Source &src, int first_round, int n_rounds) {
    std::vector<Ints> blobs;
    for (int i = first_round; i < first_round + n_rounds; ++i) {
        blobs.push_back(F.do_round(src));
        F.t.launched();
        F.tp.tick = F.t.ran[0] % 4 == 0;   // a tick every 4 frames
    }
    return blobs;
}

static bool same_log(const TextLog &a, const TextLog &b) {
    if (a.ids != b.ids || a.pieces.size() != b.pieces.size()) return false;
    for (size_t u = 0; u < a.pieces.size(); ++u) {
        if (a.pieces[u].size() != b.pieces[u].size()) return false;
        for (size_t i = 0; i < a.pieces[u].size(); ++i)
            if (a.pieces[u][i].frames != b.pieces[u][i].frames || a.pieces[u][i].n != b.pieces[u][i].n ||
                a.pieces[u][i].end != b.pieces[u][i].end)
                return false;
    }
    return true;
}

static void test_replay() {
    // utterance 0: K = 1, asked at 0 (nothing), 1 (1 id), 2 (3 ids), at the tick after frame 4 (the end); utterance 1:
    // K = 2, asked at 0 (nothing), 2 (1 id), 3 (3 ids), the tick (the end).  No ask goes unanswered at frames == K, so no
    // slot is ever held and both run every frame
    const std::vector<uint8_t> open = {1, 1};
    const Ints n_head = {5, 6}, max_len = {100, 100};
    Source live;
    live.answers = {{0, 1, {11}, false}, {0, 2, {12, 13, 14}, false}, {0, 4, {}, true},
                    {1, 2, {21}, false}, {1, 3, {22, 23, 24}, false}, {1, 4, {}, true}};
    TextLog log;
    log.ids.resize(2); log.pieces.resize(2);
    Feeds A(2, open, n_head, max_len, &log);
    const std::vector<Ints> first = run_schedule(A, live, 0, 6);
    CHECK(live.calls == (std::vector<std::pair<int, int>>{{0, 0}, {1, 0}, {0, 1}, {0, 2}, {1, 2}, {1, 3}, {0, 4}, {1, 4}}));
    CHECK(live.rows_ahead == (Ints{1, 2, 0, 0, 0, 0, 1, 2}));
    TextLog want;
    want.ids = {{11, 12, 13, 14}, {21, 22, 23, 24}};
    want.pieces = {{{1, 1, false}, {2, 3, false}, {4, 0, true}}, {{2, 1, false}, {3, 3, false}, {4, 0, true}}};
    CHECK(same_log(log, want));
    CHECK(first.size() == 6 && first[0] == (Ints{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
    CHECK(first[2] == (Ints{0, 0, 0, 0, 0, 5, 14, 1, 3, 12, 0, 0, 2, 1, 0, 3, 2, 0, 4, 3, 1, 2, 12, 13, 14, 21}));
    CHECK(first[4] == (Ints{0, 0, 0, 0, 0, 6, 14, 1, 7, 15, 0, 0, 5, 0, 1, 6, TTS_EOS}));
    CHECK(A.held == (std::vector<int32_t>{0, 0}) && A.t.ran == (Ints{6, 6}));

    // a re-run with the whole log: the same rounds, no ask
    Source none;
    none.forbidden = true;
    Feeds B(2, open, n_head, max_len, &log);
    CHECK(run_schedule(B, none, 0, 6) == first);
    CHECK(none.calls.empty() && same_log(log, want));

    // a run that breaks off after round 2 (utterance 0 has its second piece, utterance 1 its first), then a re-run:
    // the log's pieces are replayed and the callback is asked for the ones it lacks
    TextLog part;
    part.ids.resize(2); part.pieces.resize(2);
    Source s1 = live;
    s1.calls.clear(); s1.rows_ahead.clear();
    Feeds C(2, open, n_head, max_len, &part);
    const std::vector<Ints> head = run_schedule(C, s1, 0, 3);
    CHECK(head == std::vector<Ints>(first.begin(), first.begin() + 3));
    CHECK(part.ids == (std::vector<std::vector<int32_t>>{{11, 12, 13, 14}, {21}}));
    Source s2 = live;
    s2.calls.clear(); s2.rows_ahead.clear();
    Feeds D(2, open, n_head, max_len, &part);
    CHECK(run_schedule(D, s2, 0, 6) == first);
    CHECK(s2.calls == (std::vector<std::pair<int, int>>{{1, 3}, {0, 4}, {1, 4}}));
    CHECK(same_log(part, want));
}

// ---- 5. rejections, with the messages the C API hands on
static void test_rejections() {
    TextLog log;
    log.ids.resize(1); log.pieces.resize(1);
    Feeds F(1, {1}, Ints{5}, Ints{100}, &log);
    F.tp.text_vocab = 1000;
    F.tp.max_trailing = 8;
    const int32_t bad_id[2] = {5, 1000}, seven[7] = {1, 2, 3, 4, 5, 6, 7};
    CHECK(F.tp.feed_piece(0, 0, bad_id, 2, false) == "utterance 0: fed text token out of range");
    CHECK(F.tp.feed_piece(0, 0, seven, -1, false) == "utterance 0: bad text feed");
    CHECK(F.tp.feed_piece(0, 0, nullptr, 1, false) == "utterance 0: bad text feed");
    CHECK(F.tp.feed_piece(0, 0, seven, 7, false) == "utterance 0: text feed exceeds the trailing-text buffer");
    CHECK(F.tp.rows_known == (Ints{1}) && !F.tp.closed[0] && F.round.ids.empty() && F.round.rows.empty() && F.round.commit.empty());
    CHECK(F.tp.feed_piece(0, 0, seven, 6, false).empty() && F.tp.rows_known == (Ints{7}));   // K + n + 1 == max_trailing fits
    // the same through an ask: the message comes back, nothing is logged
    Source src;
    src.answers = {{0, 0, {1000}, false}};
    bool aborted = false;
    CHECK(F.tp.ask(F.t, Source::ask, &src, &aborted) == "utterance 0: fed text token out of range");
    CHECK(F.tp.rows_known == (Ints{7}) && log.ids[0].empty() && log.pieces[0].empty());

    std::vector<int32_t> padded = {42};
    const int32_t head[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    CHECK(open_head(2, head, 3, 1000, 8, 999, padded) == "utterance 2: an open utterance needs a head of at least 4 ids");
    CHECK(open_head(2, head, 12, 1000, 8, 999, padded) == "utterance 2: head too long for the trailing-text buffer");
    CHECK(open_head(2, bad_id, 2, 1000, 8, 999, padded) == "utterance 2: an open utterance needs a head of at least 4 ids");
    const int32_t bad_head[4] = {1, 2, 3, 1000};
    CHECK(open_head(2, bad_head, 4, 1000, 8, 999, padded) == "utterance 2: text token out of range");
    CHECK(padded == (std::vector<int32_t>{42}));
    CHECK(open_head(2, head, 11, 1000, 8, 999, padded).empty());   // n - 4 + 1 == max_trailing fits
    CHECK(padded == (std::vector<int32_t>{1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 999, 999, 999, 999, 999}));
}

int main() {
    test_admission_and_reap();
    test_frame_slots();
    test_text_round();
    test_replay();
    test_rejections();
    std::printf(fails ? "queue_sched: %d failures\n" : "queue_sched: ok\n", fails);
    return fails ? 1 : 0;
}
