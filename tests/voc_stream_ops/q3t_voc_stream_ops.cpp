// q3t_voc_stream_ops.cpp — test-only C entry points over the vocoder stream's attention launchers voc_kv_append() and
// voc_attn_cached() (csrc/vocoder_kernels.h), so that a test can run ONE launch on device buffers of its own and
// compare it with the whole-sequence attention and with a reference (tests/test_gpu_voc_stream_ops.py).  A library of
// its own, like tests/attn_ops/, so that the files the other op tests load stay as they are.  Not part of the product:
// nothing here is exported through include/q3t_backend.h; the library links libq3t.so and calls the q3t:: launchers on
// the null stream, then synchronises.  Every entry returns 0, or -1 with the error text in err.
#include <cstdint>
#include <cstring>
#include <string>

#include "vocoder_kernels.h"

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

// pointers are device addresses; the caller guarantees P + n rows in kc / vc / rope
int q3t_vso_kv_append(uint64_t qkv, uint64_t rope, uint64_t kc, uint64_t vc, int32_t P, int32_t n, int32_t nH, int32_t D,
                      char *err, int errlen) {
    return finish(voc_kv_append(ptr<float>(qkv), ptr<const float>(rope), ptr<float>(kc), ptr<float>(vc), P, n, nH, D, nullptr),
                  err, errlen);
}

int q3t_vso_attn_cached(uint64_t qkv, uint64_t kc, uint64_t vc, uint64_t out, int32_t P, int32_t n, int32_t nH, int32_t D,
                        char *err, int errlen) {
    return finish(voc_attn_cached(ptr<const float>(qkv), ptr<const float>(kc), ptr<const float>(vc), ptr<uint16_t>(out), P, n,
                                  nH, D, nullptr), err, errlen);
}

}  // extern "C"
