// queue_plan / queue_commit (csrc/queue_deliver.h) for utterances that are fed their text while they run: a held slot
// gains no frame between two ticks, so a tick's chunk may carry 0 .. interval frames for it.  Three slots gain 0, 1 and
// `interval` frames, rotated over three ticks, then all finish.  Asserted: no delivery without frames that is not
// final, exactly one final delivery per utterance, entries in utterance order, and the delivered counts sum to what
// the slots gained.  CPU only.
#include <cstdio>
#include <vector>

#include "queue_deliver.h"

using namespace q3t;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

int main() {
    const int S = 3, interval = 4;
    const int gain[3] = {0, 1, interval};
    QueueState st(S);
    QueueRun run(S);
    std::vector<int> stops, utt = {2, 0, 1};   // slot k runs utterance utt[k]
    std::vector<int> total(S, 0), finals(S, 0), pieces(S, 0);
    std::vector<int32_t> no_stop(S, 0);
    for (int tick = 0; tick < 3; ++tick) {
        int hdr[S];
        for (int k = 0; k < S; ++k) { hdr[k] = gain[(k + tick) % 3]; total[utt[k]] += hdr[k]; }
        std::vector<QueueEntry> ent;
        queue_plan(hdr, utt, false, st, run, ent, stops);
        CHECK(ent.size() == 2);   // the slot that gained nothing makes no delivery
        for (size_t i = 0; i < ent.size(); ++i) {
            CHECK(ent[i].n > 0 && ent[i].n <= interval && !ent[i].final && ent[i].skip == 0);
            CHECK(i == 0 || ent[i - 1].utt < ent[i].utt);
            CHECK(ent[i].n == hdr[ent[i].slot] && utt[ent[i].slot] == ent[i].utt);
            ++pieces[ent[i].utt];
        }
        queue_commit(ent, no_stop.data(), true, st, run, stops);
    }
    // the finish: one gains nothing more (its final delivery is empty), the others their rest
    int hdr[S] = {0, 2, 1};
    for (int k = 0; k < S; ++k) total[utt[k]] += hdr[k];
    std::vector<QueueEntry> ent;
    queue_plan(hdr, utt, true, st, run, ent, stops);
    CHECK(ent.size() == 3);
    for (const QueueEntry &e : ent) { CHECK(e.final == 1); ++finals[e.utt]; }
    queue_commit(ent, no_stop.data(), true, st, run, stops);
    // a collection after the final one hands nothing out
    queue_plan(hdr, utt, false, st, run, ent, stops);
    CHECK(ent.empty());
    for (int u = 0; u < S; ++u) {
        CHECK(finals[u] == 1 && st.finaled[u] && !st.stopped[u]);
        CHECK(st.delivered[u] == total[u]);
        CHECK(pieces[u] == 2);   // of three ticks, one found the slot without a new frame
    }
    CHECK(stops.empty() && !st.aborted);
    std::printf(fails ? "queue_plan text: %d failures\n" : "queue_plan text: ok\n", fails);
    return fails ? 1 : 0;
}
