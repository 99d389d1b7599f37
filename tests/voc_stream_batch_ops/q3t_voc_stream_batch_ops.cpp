// q3t_voc_stream_batch_ops.cpp — test-only C entry points over the batched vocoder-stream attention launchers
// voc_kv_append_batch() and voc_attn_cached_batch() (csrc/vocoder_kernels.h), so that a test can run ONE batched launch
// on device buffers of its own and compare it, stream by stream, with the single-stream launchers
// (tests/test_gpu_voc_stream_batch_ops.py).  A library of its own, like tests/voc_stream_ops/, so that the files the
// other op tests load stay as they are.  Not part of the product: nothing here is exported through
// include/q3t_backend.h; the library links libq3t.so and calls the q3t:: launchers on the null stream, then
// synchronises.  Every entry returns 0, or -1 with the error text in err.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "vocoder_kernels.h"

using namespace q3t;

namespace {

template <typename T> T *ptr(uint64_t v) { return reinterpret_cast<T *>(static_cast<uintptr_t>(v)); }

int fail(const std::string &msg, char *err, int errlen) {
    if (err && errlen > 0) {
        std::strncpy(err, msg.c_str(), (size_t)errlen - 1);
        err[errlen - 1] = 0;
    }
    return -1;
}

// the caller's descriptors (host memory, device addresses inside) -> a device array for the launch
struct HostDesc { uint64_t kc, vc, rope; int64_t layer_stride; int32_t P, n, row0, pad_; };
static_assert(sizeof(HostDesc) == sizeof(VocStreamDesc), "descriptor layout");

struct DevDescs {
    VocStreamDesc *d = nullptr;
    int max_n = 0, max_tiles = 0;
    bool upload(const HostDesc *h, int ns, std::string *msg) {
        std::vector<VocStreamDesc> v((size_t)std::max(ns, 0));
        for (int j = 0; j < ns; ++j) {
            v[j].kc = ptr<float>(h[j].kc); v[j].vc = ptr<float>(h[j].vc); v[j].rope = ptr<const float>(h[j].rope);
            v[j].layer_stride = h[j].layer_stride; v[j].P = h[j].P; v[j].n = h[j].n; v[j].row0 = h[j].row0;
            max_n = std::max(max_n, h[j].n);
            max_tiles = std::max(max_tiles, (h[j].P + h[j].n + 31) / 32 - h[j].P / 32);
        }
        if (hipMalloc((void **)&d, std::max<size_t>(v.size() * sizeof(VocStreamDesc), 16)) != hipSuccess ||
            hipMemcpy(d, v.data(), v.size() * sizeof(VocStreamDesc), hipMemcpyHostToDevice) != hipSuccess) {
            *msg = "descriptor upload failed";
            return false;
        }
        return true;
    }
    ~DevDescs() { if (d) hipFree(d); }
};

int finish(bool ok, char *err, int errlen) {
    if (!ok) return fail(last_error(), err, errlen);
    const hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) return 0;
    return fail(std::string("hipDeviceSynchronize: ") + hipGetErrorString(e), err, errlen);
}

}  // namespace

extern "C" {

// pointers are device addresses; the caller guarantees P + n rows in every stream's kc / vc (of every layer) / rope
int q3t_vsbo_kv_append_batch(uint64_t qkv, const void *descs, int32_t n_streams, int32_t layer, int32_t nH, int32_t D,
                             char *err, int errlen) {
    DevDescs dd;
    std::string msg;
    if (!dd.upload(static_cast<const HostDesc *>(descs), n_streams, &msg)) return fail(msg, err, errlen);
    return finish(voc_kv_append_batch(ptr<float>(qkv), dd.d, n_streams, dd.max_n, layer, nH, D, nullptr), err, errlen);
}

int q3t_vsbo_attn_cached_batch(uint64_t qkv, uint64_t out, const void *descs, int32_t n_streams, int32_t layer, int32_t nH,
                               int32_t D, char *err, int errlen) {
    DevDescs dd;
    std::string msg;
    if (!dd.upload(static_cast<const HostDesc *>(descs), n_streams, &msg)) return fail(msg, err, errlen);
    return finish(voc_attn_cached_batch(ptr<const float>(qkv), ptr<uint16_t>(out), dd.d, n_streams, dd.max_tiles, layer, nH, D,
                                        nullptr), err, errlen);
}

// n_copies independent copies of n floats each in one launch
int q3t_vsbo_copy_batch(const uint64_t *src, const uint64_t *dst, const int64_t *n, int32_t n_copies, char *err, int errlen) {
    std::vector<VocCopyDesc> v((size_t)std::max(n_copies, 0));
    int64_t max_n = 0;
    bool vec4 = true;
    for (int j = 0; j < n_copies; ++j) {
        v[j].src = ptr<const float>(src[j]); v[j].dst = ptr<float>(dst[j]); v[j].n = n[j];
        max_n = std::max(max_n, n[j]);
        vec4 = vec4 && n[j] % 4 == 0 && src[j] % 16 == 0 && dst[j] % 16 == 0;
    }
    VocCopyDesc *d = nullptr;
    if (hipMalloc((void **)&d, std::max<size_t>(v.size() * sizeof(VocCopyDesc), 16)) != hipSuccess ||
        hipMemcpy(d, v.data(), v.size() * sizeof(VocCopyDesc), hipMemcpyHostToDevice) != hipSuccess) {
        if (d) hipFree(d);
        return fail("descriptor upload failed", err, errlen);
    }
    const int rc = finish(voc_copy_batch(d, n_copies, max_n, vec4, nullptr), err, errlen);
    hipFree(d);
    return rc;
}

}  // extern "C"
