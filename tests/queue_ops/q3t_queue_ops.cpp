// q3t_queue_ops.cpp — test-only C entry point over the continuous-batching queue's collection launcher
// queue_collect() (csrc/kernels.h), so that a test can run ONE launch on device buffers of its own and compare it with
// a numpy restatement (tests/test_gpu_queue_collect_ops.py).  A library of its own, like tests/voc_stream_ops/, so
// that the files the other op tests load stay as they are.  Not part of the product: nothing here is exported through
// include/q3t_backend.h; the library links libq3t.so and calls the q3t:: launcher on the null stream, then
// synchronises.  The entry returns 0, or -1 with the error text in err.
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

// pointers are device addresses: mask / done / frame / delivered / header [S], codes [S][codes_max_len][16],
// rows [S][interval][16], error [1]
int q3t_qo_collect(uint64_t mask, uint64_t done, uint64_t frame, uint64_t delivered, uint64_t codes, uint64_t rows,
                   uint64_t header, uint64_t error, int32_t S, int32_t interval, int32_t codes_max_len, int32_t max_len,
                   char *err, int errlen) {
    QueueCollect q;
    q.mask = ptr<const int>(mask); q.done = ptr<const int>(done); q.frame = ptr<const int>(frame);
    q.delivered = ptr<int>(delivered);
    q.codes = ptr<const int32_t>(codes);
    q.rows = ptr<int32_t>(rows);
    q.header = ptr<int>(header); q.error = ptr<int>(error);
    q.interval = interval; q.codes_max_len = codes_max_len; q.max_len = max_len;
    return finish(queue_collect(q, S, nullptr), err, errlen);
}

}  // extern "C"
