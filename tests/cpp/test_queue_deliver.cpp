// test_queue_deliver.cpp — the host bookkeeping of the queue's deliveries (csrc/queue_deliver.h) on the CPU: a scripted
// queue of chunks goes through queue_plan / queue_commit as Engine::QueueStreamer drives them, once straight through and
// once "faulting" after every possible number of chunks and re-running from the start with the QueueState kept.  In
// every case the callback must see, per utterance, exactly the frames of the straight run, each once and in order,
// one final (unless cancelled), nothing after a cancel; and a cancelled utterance must be cancelled again in the re-run
// no later than where it stood.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "queue_deliver.h"

using namespace q3t;

namespace {

struct Chunk { std::vector<int> utt, header; bool final; };
struct Seen { std::vector<int> frames; int finals = 0; };   // frames: the absolute frame indices handed out

int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// two slots, interval 4.  utterance 0: 10 frames, 1: 3 frames (ends before its first tick), 2: 6 frames in slot 1
// after utterance 1, 3: 5 frames, cancelled by the callback at its first piece
std::vector<Chunk> script() {
    return {
        {{0, 1}, {4, 3}, false},      // tick: utterance 1 has already ended with 3 frames
        {{-1, 1}, {0, 0}, true},      // finish of utterance 1 (nothing new)
        {{0, 2}, {4, 2}, false},      // tick
        {{0, 2}, {2, 4}, false},      // tick: utterance 0 ended at 10
        {{0, -1}, {0, 0}, true},      // finish of utterance 0
        {{3, 2}, {2, 0}, false},      // tick: utterance 3 in slot 0, cancelled here
        {{3, -1}, {3, 0}, false},     // a piece of utterance 3 still in flight: dropped
        {{-1, 2}, {0, 0}, true},      // finish of utterance 2
    };
}

// runs chunks [0, upto) of the script (utterance 3 is cancelled at its first piece); cancelled_at_run[u]: the frames
// utterance u had collected in this run when its cancel was issued
void run(int upto, QueueState &st, std::map<int, Seen> &seen, std::vector<int> &cancelled_at_run) {
    const std::vector<Chunk> sc = script();
    QueueRun r(4);
    std::vector<int> pos(4, 0);   // frames collected per utterance in this run (what the device counter stands for)
    std::vector<int> stops;
    for (int i = 0; i < upto; ++i) {
        const Chunk &c = sc[i];
        const std::vector<int> &utt = c.utt;
        std::vector<QueueEntry> ent;
        queue_plan(c.header.data(), utt, c.final, st, r, ent, stops);
        std::vector<int> before = pos;
        for (size_t k = 0; k < utt.size(); ++k) if (utt[k] >= 0) pos[utt[k]] += c.header[k];
        std::vector<int32_t> stop(ent.size(), 0);
        for (size_t j = 0; j < ent.size(); ++j) {
            const QueueEntry &e = ent[j];
            CHECK(j == 0 || ent[j - 1].utt < e.utt, "entries not in increasing utterance order");
            CHECK(e.n >= (e.final ? 0 : 1) && e.skip >= 0 && e.skip + e.n <= c.header[e.slot], "entry out of its rows");
            for (int f = 0; f < e.n; ++f) seen[e.utt].frames.push_back(before[e.utt] + e.skip + f);
            seen[e.utt].finals += e.final;
            if (e.utt == 3 && !e.final) stop[j] = 1;
        }
        queue_commit(ent, stop.data(), true, st, r, stops);
        for (int u : stops) cancelled_at_run[u] = pos[u];
        stops.clear();
    }
}

void check(const std::map<int, Seen> &seen, const QueueState &st, const char *tag) {
    const int want[4] = {10, 3, 6, 2};
    for (int u = 0; u < 4; ++u) {
        auto it = seen.find(u);
        CHECK(it != seen.end(), "%s: utterance %d never delivered", tag, u);
        if (it == seen.end()) continue;
        const Seen &s = it->second;
        CHECK((int)s.frames.size() == want[u], "%s: utterance %d got %d frames, want %d", tag, u, (int)s.frames.size(), want[u]);
        for (size_t f = 0; f < s.frames.size(); ++f) CHECK(s.frames[f] == (int)f, "%s: utterance %d frame %d out of order or twice", tag, u, (int)f);
        CHECK(s.finals == (u == 3 ? 0 : 1), "%s: utterance %d had %d finals", tag, u, s.finals);
        CHECK(st.delivered[u] == want[u], "%s: delivered[%d] = %d", tag, u, st.delivered[u]);
        CHECK(st.stopped[u] == (u == 3) && st.finaled[u] == (u != 3), "%s: flags of utterance %d", tag, u);
    }
}

}  // namespace

int main() {
    const int N = (int)script().size();
    {
        QueueState st(4);
        std::map<int, Seen> seen;
        std::vector<int> at(4, -1);
        run(N, st, seen, at);
        check(seen, st, "straight");
        CHECK(at[3] == 2, "utterance 3 cancelled at %d", at[3]);
    }
    for (int cut = 0; cut <= N; ++cut) {   // a fault after `cut` delivered chunks, then the whole queue again
        QueueState st(4);
        std::map<int, Seen> seen;
        std::vector<int> at(4, -1), at2(4, -1);
        run(cut, st, seen, at);
        run(N, st, seen, at2);
        char tag[32];
        snprintf(tag, sizeof tag, "fault after %d", cut);
        check(seen, st, tag);
        // cancelled before the fault: cancelled again, without a callback, as soon as it stands where it stood
        if (at[3] >= 0) CHECK(at2[3] == 2, "%s: utterance 3 cancelled again at %d", tag, at2[3]);
    }
    {   // an abort is recorded and changes nothing else
        QueueState st(2);
        QueueRun r(2);
        std::vector<QueueEntry> ent;
        std::vector<int> stops;
        const int hdr[2] = {4, 1};
        queue_plan(hdr, {0, 1}, false, st, r, ent, stops);
        const int32_t stop[2] = {0, 0};
        queue_commit(ent, stop, false, st, r, stops);
        CHECK(st.aborted && st.delivered[0] == 4 && st.delivered[1] == 1 && stops.empty(), "abort bookkeeping");
    }
    if (fails) printf("%d checks failed\n", fails);
    else printf("queue_deliver: all checks passed\n");
    return fails ? 1 : 0;
}
