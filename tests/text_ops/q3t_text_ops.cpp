// q3t_text_ops.cpp — test-only C entry points over the text-feed launchers text_append() / slot_hold() /
// slot_release() (csrc/kernels.h), so that a test can run ONE launch on device buffers of its own and compare it with a
// numpy restatement (tests/test_gpu_text_ops.py).  A library of its own, like tests/queue_ops/.  Not part of the
// product: nothing here is exported through include/q3t_backend.h; the library links libq3t.so and calls the q3t::
// launchers on the null stream, then synchronises.  An entry returns 0, or -1 with the error text in err.
#include <cstdint>
#include <cstring>
#include <string>

#include "kernels.h"

using namespace q3t;

namespace {

template <typename T> T *ptr(uint64_t v) { return reinterpret_cast<T *>(static_cast<uintptr_t>(v)); }

int finish(bool ok, char *err, int errlen) {
    std::string msg;
    if (!ok) msg = last_error();
    else {
        const hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) return 0;
        msg = std::string("hipDeviceSynchronize: ") + hipGetErrorString(e);
    }
    if (err && errlen > 0) {
        std::strncpy(err, msg.c_str(), (size_t)errlen - 1);
        err[errlen - 1] = 0;
    }
    return -1;
}

}  // namespace

extern "C" {

// pointers are device addresses: src [src_rows][H], trailing [S][max_trailing][H], rows [n_rows][3], commit
// [n_commit][3], trailing_len / n_tokens [S], error [1]
int q3t_to_append(uint64_t src, uint64_t trailing, uint64_t rows, uint64_t commit, uint64_t trailing_len, uint64_t n_tokens,
                  uint64_t error, int32_t n_rows, int32_t n_commit, int32_t src_rows, int32_t S, int32_t max_trailing,
                  int32_t H, char *err, int errlen) {
    TextAppend t;
    t.src = ptr<const float>(src); t.trailing = ptr<float>(trailing);
    t.rows = ptr<const int>(rows); t.commit = ptr<const int>(commit);
    t.trailing_len = ptr<int>(trailing_len); t.n_tokens = ptr<int>(n_tokens); t.error = ptr<int>(error);
    t.n_rows = n_rows; t.n_commit = n_commit; t.src_rows = src_rows; t.S = S; t.max_trailing = max_trailing; t.H = H;
    return finish(text_append(t, nullptr), err, errlen);
}

// mask / done / held / frame [S], hidden / save [S][H]; release != 0: slot_release, else slot_hold
int q3t_to_hold(uint64_t mask, uint64_t hidden, uint64_t save, uint64_t done, uint64_t held, uint64_t frame, int32_t S,
                int32_t H, int32_t release, char *err, int errlen) {
    SlotHold h;
    h.mask = ptr<const int>(mask); h.hidden = ptr<float>(hidden); h.save = ptr<float>(save);
    h.done = ptr<int>(done); h.held = ptr<int>(held); h.frame = ptr<const int>(frame); h.H = H;
    return finish(release ? slot_release(h, S, nullptr) : slot_hold(h, S, nullptr), err, errlen);
}

}  // extern "C"
