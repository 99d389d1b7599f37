// queue_deliver.h — the host bookkeeping of the queue's deliveries (generate_queue with a callback; DESIGN 2f "Queue
// deliveries"): which entries of a collected chunk go to the callback, and what the callback's answer changes.
// Header-only and free of HIP so tests/cpp/test_queue_deliver.cpp drives it on the CPU, the fallback re-run included
// (a re-run generates every utterance again from frame 0 and must hand nothing out twice).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace q3t {

struct QueueState {   // per utterance, kept across a fallback re-run of the queue
    std::vector<int> delivered;            // frames handed to the callback
    std::vector<char> stopped, finaled;    // cancelled by the callback; its final delivery was made
    bool aborted = false;                  // the callback returned 0
    explicit QueueState(int n_utt = 0) : delivered(n_utt, 0), stopped(n_utt, 0), finaled(n_utt, 0) {}
};

struct QueueRun {   // per utterance, of one run of the queue
    std::vector<int> run;      // frames collected in this run
    std::vector<char> gone;    // no further delivery in this run: final made, or cancelled
    explicit QueueRun(int n_utt = 0) : run(n_utt, 0), gone(n_utt, 0) {}
};

struct QueueEntry { int utt, slot, skip, n, final; };   // rows [skip, skip + n) of the slot's chunk rows

// One collected chunk: header[k] = frames collected for slot k, utt[k] = the slot's utterance (-1: not selected).
// Fills ent (increasing utt) with what goes to the callback and appends to stops the utterances whose slots must be
// cancelled without a callback (re-run of an utterance cancelled before the fault, once it stands where it stood).
inline void queue_plan(const int *header, const std::vector<int> &utt, bool final, const QueueState &st, QueueRun &r,
                       std::vector<QueueEntry> &ent, std::vector<int> &stops) {
    ent.clear();
    for (int k = 0; k < (int)utt.size(); ++k) {
        const int u = utt[k];
        if (u < 0 || r.gone[u]) continue;
        int n = header[k];
        const int before = r.run[u];
        r.run[u] += n;
        if (st.finaled[u]) { r.gone[u] = final; continue; }   // re-run of a finished utterance: silent
        if (st.stopped[u]) {                                  // re-run of a cancelled one: cancel it where it stood
            if (final || r.run[u] >= st.delivered[u]) { r.gone[u] = 1; if (!final) stops.push_back(u); }
            continue;
        }
        const int skip = std::min(n, std::max(0, st.delivered[u] - before));   // delivered before the fault
        n -= skip;
        if (n == 0 && !final) continue;
        ent.push_back(QueueEntry{u, k, skip, n, final ? 1 : 0});
    }
    std::sort(ent.begin(), ent.end(), [](const QueueEntry &a, const QueueEntry &b) { return a.utt < b.utt; });
}

// The callback has seen ent: stop[i] != 0 cancels ent[i].utt (ignored on its final delivery), go == false aborts.
inline void queue_commit(const std::vector<QueueEntry> &ent, const int32_t *stop, bool go, QueueState &st, QueueRun &r,
                         std::vector<int> &stops) {
    for (size_t i = 0; i < ent.size(); ++i) {
        const int u = ent[i].utt;
        st.delivered[u] += ent[i].n;
        if (ent[i].final) { st.finaled[u] = 1; r.gone[u] = 1; }
        else if (stop[i]) { st.stopped[u] = 1; r.gone[u] = 1; stops.push_back(u); }
    }
    if (!go) st.aborted = true;
}

}  // namespace q3t
