// speaker.h — MI355X-native speaker encoder (ECAPA-TDNN) replacing AudioTokenizerEncoder
// (src/audio_tokenizer_encoder.{h,cpp}): log-mel front end as two f32 GEMMs (DFT basis, mel filterbank) instead of the
// reference's O(n_fft^2)-per-frame naive DFT (:96-106), then the SE-Res2Net / MFA / ASP / FC graph (:438-694) on the
// vocoder's implicit-GEMM conv kernels.  Activations are time-major [T][C] f32; every conv input is rounded to f16
// (ggml_conv_1d's F16 im2col) against the GGUF's F16 weights.
#pragma once
#include <string>
#include <vector>

#include "arena.h"
#include "gguf.h"
#include "vocoder_kernels.h"

namespace q3t {

// One clip of a ragged batch (SpeakerEncoder::encode_batch): its samples start sample_off floats into the packed sample
// buffer, its T mel frames own rows row0 .. row0 + T - 1 of every time-major activation buffer, followed by GAP rows
// nobody reads.  One device array of these describes the batch to every ragged kernel.
struct SpkClip { int32_t sample_off, n, row0, T; };
// kernel launches of the encoder so far, process-wide (every launch counts; a conv is its pad launch and its conv launch)
int64_t speaker_launches();

class SpeakerEncoder {
public:
    ~SpeakerEncoder();
    // weights from the TTS GGUF (spk_enc.*) into `wa` (the context's weight blob: broadcast with it); false + error
    // when the tensors are absent or malformed
    bool load(const Gguf &g, WeightArena &wa, hipStream_t s);
    bool loaded() const { return loaded_; }
    int dim() const { return dim_; }
    int sample_rate() const { return sample_rate_; }
    // AudioTokenizerEncoder::encode (audio_tokenizer_encoder.h:107-108): samples in [-1, 1] at 24 kHz -> emb [dim()]
    bool encode(const float *samples, int n, float *emb);
    // n_clips clips of any lengths through shared launches: emb [n_clips][dim()], row c bit for bit encode(samples[c],
    // n[c]) whatever its neighbours, its position and the batch size.  Clips are packed in order, GAP rows apart, into
    // groups of at most Q3T_SPK_GROUP_ROWS packed rows (default 4096, read at each call): below the row count at which
    // conv_kernel() would pick another kernel instance than for the clip alone (checked per group on the host; a group
    // that fails the check, and a clip longer than a group, go through encode()).  A clip with fewer than 5 mel frames
    // gets ok[c] = 0 and a zeroed row and takes no rows; with ok == nullptr it fails the call before any device work.
    bool encode_batch(const float *const *samples, const int *n, int n_clips, float *emb, int *ok);
    // mel spectrogram [n_frames][128] (time-major; test entry point)
    bool mel(const float *samples, int n, std::vector<float> &mel, int *n_frames);

private:
    struct Conv { uint16_t *w = nullptr; float *b = nullptr; int k = 0, ic = 0, oc = 0; };   // w [k][oc][ic]
    static constexpr int GAP = 8;     // rows between two clips: twice the largest reflect pad (4)
    static constexpr int VS = 8192;   // floats of one clip's vectors (SE mean / gates, ASP statistics, pooled, result)
    static int group_rows();
    bool ensure(int T);               // scratch for T rows (a clip's frames or a batch's packed rows)
    bool upload(const float *samples, int n);   // host samples -> samples_ (grown on demand)
    bool run_mel(const float *samples_dev, int n, int F);
    bool graph(const float *samples_dev, int n, int T);
    bool encode_group(const float *const *samples, const int *n, const int *T, const int *idx, int g, int cap_rows,
                      float *emb);
    ConvParams conv_params(const Conv &c, int M, int T_in, int dil, float *y, int ldy, int act) const;
    bool same_conv_kernels(int R, int T) const;
    // valid conv over a reflect-padded f16 copy of x[T][ldx] (pad rows each side; optional x2 added first)
    bool conv(const Conv &c, const float *x, int ldx, const float *x2, int ldx2, int T, int pad, int dil, float *y,
              int ldy, int act);
    template <class T> T *dalloc(size_t n);

    bool loaded_ = false;
    hipStream_t stream_ = nullptr;
    int dim_ = 0, sample_rate_ = 24000;
    Conv conv0_, mfa_, asp_tdnn_, asp_conv_, fc_;
    struct Blk { Conv tdnn1, tdnn2, res[7], se1, se2; } blk_[3];
    std::vector<void *> allocs_, scratch_;
    float *basis_ = nullptr, *fb_ = nullptr, *win_ = nullptr;   // DFT basis [1024][1026], filterbank [513][128], Hann
    int cap_T_ = 0, cap_n_ = 0;
    float *samples_ = nullptr;
    float *frames_ = nullptr, *spec_ = nullptr, *mag_ = nullptr, *mel_ = nullptr;
    float *x0_ = nullptr, *h_ = nullptr, *cat_ = nullptr, *y_ = nullptr, *mfa_out_ = nullptr, *blocks_ = nullptr,
          *att_ = nullptr, *att2_ = nullptr, *vec_ = nullptr;
    uint16_t *xh_ = nullptr;   // f16 conv input (reflect-padded copy / ASP [hs | mean | std])
    // ragged batch: set while a group runs (null: the single-clip launches)
    const SpkClip *clips_ = nullptr;
    int n_clips_ = 0, max_T_ = 0;
    float *bbuf_ = nullptr, *bvec_ = nullptr;   // [descriptors | packed samples]; per-clip vectors [clips][VS]
    size_t bbuf_cap_ = 0;
    int bvec_cap_ = 0;
    std::vector<float> host_, out_;
};

}  // namespace q3t
