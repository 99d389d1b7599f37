// q3t_pcm_ops.cpp — test-only C entry point over the output stage's launchers pcm_out() and pcm_out_hist()
// (csrc/pcm_out.h), so that a test can run k_pcm_out alone on raw f32 input of its own: any number of streams in ONE
// launch, each with its rate, format, position, carried history and an output buffer placed at a byte offset of the
// test's choosing inside a poisoned region (tests/test_gpu_pcm_ops.py).  A library of its own, like
// tests/voc_stream_batch_ops/.  Not part of the product: nothing here is exported through include/q3t_backend.h; the
// library links libq3t.so, calls the q3t:: launchers on the null stream and synchronises.  Returns 0, or -1 with the
// error text in err.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pcm_out.h"
#include "q3t_common.h"

using namespace q3t;

namespace {

int fail(const std::string &msg, char *err, int errlen) {
    if (err && errlen > 0) {
        std::strncpy(err, msg.c_str(), (size_t)errlen - 1);
        err[errlen - 1] = 0;
    }
    return -1;
}

struct DevMem {   // every device allocation of a call, freed when it ends
    std::vector<void *> ptrs;
    void *get(size_t bytes) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
    ~DevMem() { for (void *p : ptrs) hipFree(p); }
};

}  // namespace

extern "C" {

// One launch of k_pcm_out (and one of the history update) over n streams.  All pointers are HOST pointers.
//   x[j]        n_in[j] new input samples of stream j
//   hist[j]     kPcmMaxHist floats, in and out: the carried history (its first K - 1 entries are used)
//   s0[j]       input samples the stream has consumed before this launch; the outputs before it follow from the formula
//   final[j]    the push carries the tail
//   region[j]   region_bytes[j] bytes, in and out: uploaded as they are, the stream's output written from byte
//               out_off[j] on, the whole region copied back -- so the test sees every byte around the output
//   n_out[j]    receives the output count
int q3t_pcmo_run(int32_t n, const float *const *x, const int32_t *n_in, float *const *hist, const int32_t *rate,
                 const int32_t *format, const int64_t *s0, const int32_t *final, uint8_t *const *region,
                 const int64_t *region_bytes, const int64_t *out_off, int64_t *n_out, char *err, int errlen) {
    if (n <= 0) return fail("n must be > 0", err, errlen);
    DevMem mem;
    std::vector<PcmOutDesc> d((size_t)n);
    std::vector<void *> dreg((size_t)n);
    int64_t max_out = 0;
    for (int j = 0; j < n; ++j) {
        PcmRate g;
        std::vector<float> taps;
        const int bps = pcm_bytes_per_sample(format[j]);
        if (!pcm_taps(rate[j], &g, &taps) || !bps) return fail("stream " + std::to_string(j) + ": bad rate or format", err, errlen);
        const int64_t before = pcm_num_samples(s0[j], rate[j], false);
        const int64_t after = pcm_num_samples(s0[j] + n_in[j], rate[j], final[j] != 0);
        n_out[j] = after - before;
        // the bounds the kernel relies on: the output inside the region, aligned to its sample size
        if (out_off[j] < 0 || out_off[j] % bps || out_off[j] + n_out[j] * bps > region_bytes[j])
            return fail("stream " + std::to_string(j) + ": output does not fit its region", err, errlen);
        float *dx = (float *)mem.get((size_t)n_in[j] * 4), *dh = (float *)mem.get(kPcmMaxHist * 4);
        float *dt = (float *)mem.get(taps.size() * 4);
        dreg[j] = mem.get((size_t)region_bytes[j]);
        if (!dx || !dh || !dt || !dreg[j]) return fail("device alloc failed", err, errlen);
        if ((n_in[j] && hipMemcpy(dx, x[j], (size_t)n_in[j] * 4, hipMemcpyHostToDevice) != hipSuccess) ||
            hipMemcpy(dh, hist[j], kPcmMaxHist * 4, hipMemcpyHostToDevice) != hipSuccess ||
            (!taps.empty() && hipMemcpy(dt, taps.data(), taps.size() * 4, hipMemcpyHostToDevice) != hipSuccess) ||
            (region_bytes[j] && hipMemcpy(dreg[j], region[j], (size_t)region_bytes[j], hipMemcpyHostToDevice) != hipSuccess))
            return fail("upload failed", err, errlen);
        PcmOutDesc &q = d[j];
        q.x = dx; q.hist = dh; q.taps = dt; q.out = (uint8_t *)dreg[j] + out_off[j];
        q.s0 = s0[j]; q.n0 = before; q.n_in = n_in[j]; q.n_out = (int32_t)n_out[j];
        q.n_zero = final[j] ? g.D : 0;
        q.L = g.L; q.M = g.M; q.K = g.K; q.format = format[j];
        max_out = std::max(max_out, n_out[j]);
    }
    PcmOutDesc *dd = (PcmOutDesc *)mem.get(d.size() * sizeof(PcmOutDesc));
    if (!dd || hipMemcpy(dd, d.data(), d.size() * sizeof(PcmOutDesc), hipMemcpyHostToDevice) != hipSuccess)
        return fail("descriptor upload failed", err, errlen);
    if (!pcm_out(dd, n, max_out, nullptr) || !pcm_out_hist(dd, n, nullptr)) return fail(last_error(), err, errlen);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(std::string("hipDeviceSynchronize: ") + hipGetErrorString(e), err, errlen);
    for (int j = 0; j < n; ++j)
        if (hipMemcpy(hist[j], d[j].hist, kPcmMaxHist * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            (region_bytes[j] && hipMemcpy(region[j], dreg[j], (size_t)region_bytes[j], hipMemcpyDeviceToHost) != hipSuccess))
            return fail("download failed", err, errlen);
    return 0;
}

}  // extern "C"
