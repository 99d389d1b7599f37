// pcm_out.h — the output stage: the vocoder's f32 samples resampled by a causal polyphase FIR and written as f32, s16
// or G.711 mu-law, chunk-invariantly (DESIGN 2c "Output stage").  No reference counterpart: the reference's only
// conversion is the host loop of save_audio_file (cpp/qwen3_tts_pipeline.cpp), whose s16 rule is restated here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace q3t {

constexpr int kPcmF32 = 0, kPcmS16 = 1, kPcmMulaw = 2;
constexpr int kPcmNativeRate = 24000;   // the input rate the filters are designed for
constexpr int kPcmZ = 16;               // zero crossings of the prototype on each side
constexpr int kPcmMaxHist = 96;         // the longest carried history, K - 1 at 8000 Hz

// ---- host-only design (no device touched)
// The polyphase geometry of `rate` from 24000: false for a rate outside the supported list.  K = 0 at 24000 (bypass).
struct PcmRate { int L = 1, M = 1, K = 0, D = 0; };   // up, down, taps per phase, zero samples appended by `final`
bool pcm_rate(int rate, PcmRate *out);
const char *pcm_rates_text();           // "8000, 12000, ..." for messages
int pcm_bytes_per_sample(int format);   // 4 / 2 / 1, 0 for an unknown format
// outputs after n_in_total input samples: ceil((n_in_total + (final ? D : 0)) * L / M); -1 for an unsupported rate
int64_t pcm_num_samples(int64_t n_in_total, int rate, bool final);
// taps[p][k] = (float)(L * h[p + k * L]), [L][K] row-major (empty at 24000)
bool pcm_taps(int rate, PcmRate *geo, std::vector<float> *taps);

// ---- device
// One stream's share of a launch.  The stream has consumed s0 input samples and produced n0 outputs before it; x holds
// n_in new samples, followed by as many zeros as the outputs ask for (the `final` tail); hist holds the K - 1 samples
// before x (zeros at the start of a stream).  Output n (global) reads input floor(n * M / L) and the K - 1 before it.
struct PcmOutDesc {
    const float *x = nullptr;      // [n_in] new input samples (device)
    float *hist = nullptr;         // [K - 1] carried history (device); read by pcm_out, rewritten by pcm_out_hist
    const float *taps = nullptr;   // [L][K] (device); unused when K == 0
    void *out = nullptr;           // n_out samples of `format` (device), aligned to its sample size
    int64_t s0 = 0, n0 = 0;        // global index of x[0], global index of the first output
    int32_t n_in = 0, n_out = 0;
    int32_t n_zero = 0;            // zeros appended after x for the history update (D on a final push)
    int32_t L = 1, M = 1, K = 0, format = 0, pad_ = 0;
};
constexpr int kPcmBlockOut = 1024;   // outputs per workgroup (256 threads x 4)
// descs: a device array of n_streams descriptors; max_out: the largest n_out over them.  ONE launch of k_pcm_out for
// all streams; every output sample is the pinned fmaf chain of its own stream, so its bits do not depend on the batch
// around it or on how the input was cut.  Does not touch hist.
bool pcm_out(const PcmOutDesc *descs, int n_streams, int64_t max_out, hipStream_t s);
// hist <- the last K - 1 samples of [hist | x | n_zero zeros], for every stream, in one launch after pcm_out
bool pcm_out_hist(const PcmOutDesc *descs, int n_streams, hipStream_t s);
// launches of k_pcm_out by this process so far (the launch-count figure of the stage's cost)
int64_t pcm_out_launches();

}  // namespace q3t
