// vocoder.h — MI355X-native Qwen3-TTS tokenizer decoder ("vocoder"), replacing TRTVocoderDecoder
// (src/trt_vocoder.cpp) and the GGML AudioTokenizerDecoder (src/audio_tokenizer_decoder.cpp).
#pragma once
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "arena.h"
#include "gguf.h"
#include "kernels.h"
#include "pcm_out.h"

namespace q3t {

class Vocoder {
public:
    ~Vocoder();
    bool load(const std::string &tok_gguf, hipStream_t s, bool recv_weights = false);
    WeightArena &weights() { return wa_; }
    // mode 0 = FULL (GGML decoder semantics), 1 = CHUNK40 (TRT streaming semantics)
    int64_t n_samples(int n_frames, int mode) const;
    // chunk_frames: the fixed chunk length of the chunked mode (TRTVocoderDecoder::load_engine's fixed_frames)
    bool decode(const int32_t *codes_host, int n_frames, int mode, float *pcm_host, int64_t *n_out, int chunk_frames = 40);
    // n_utt utterances through shared launches: FULL decodes run as utterance batches (every conv / attention launch
    // covers up to batch_frames() frames of utterances padded to the batch's longest; the decoder is causal end to end,
    // so each utterance's samples are exactly its own decode's); CHUNK40 decodes every chunk of every utterance as one
    // batch of independent chunk_frames-long sequences.  pcm[u] capacity >= n_samples(n_frames[u], mode)
    bool decode_batch(int n_utt, const int32_t *const *codes_host, const int *n_frames, int mode, float *const *pcm_host,
                      int64_t *n_out, int chunk_frames = 40);
    // FULL decode of device-resident codes [nb][F][16] into pcm_dev [nb][n_samples(F, 0)]; ensure(F, nb) first
    bool decode_device(const int32_t *codes_dev, int n_frames, float *pcm_dev, int64_t *n_out, hipStream_t s, int nb = 1);
    bool ensure(int n_frames, int nb = 1, size_t rows = 0);
    // frames per batched launch sequence (utterances x frames); scratch grows to this (~3 MB per frame)
    int batch_frames() const { return batch_frames_; }
    void set_batch_frames(int f) { batch_frames_ = f > 0 ? f : 4096; }
    bool loaded() const { return loaded_; }
    int n_usage_normalised() const { return n_usage_; }
    // algorithmic FLOPs of one FULL decode of F frames: 2*M*K*N over every conv (per tap), transposed conv, projection
    // and the causal attention (QK^T + PV over the lower triangle), from the loaded shapes
    double decode_flops(int n_frames) const;   // codebooks divided by *.usage at load (0 for converter output)

    // ---- streaming FULL decode: frames pushed in pieces of any size; the concatenated PCM of the pushes is, bit for
    // bit, decode(all frames, mode 0).  The frame-rate part (RVQ .. output_proj) runs on the new rows only, against
    // carried state; the convolution stack is recomputed over a window of `halo` earlier frames plus the new ones and
    // the halo's samples are dropped (DESIGN 2c "Vocoder stream").  Several streams may be open; each owns its state,
    // all share the decoder's scratch and serialise on its stream.
    struct Stream {
        Vocoder *owner = nullptr;
        int device = 0;          // of the owning context (the C ABI's device lock)
        int max_frames = 0, halo = 0;
        int frames = 0;          // frames pushed so far (P)
        int64_t samples = 0;     // samples emitted so far = n_samples(frames, 0)
        float *kc = nullptr;     // [layers][max_frames][latent] f32 rotated keys
        float *vc = nullptr;     // [layers][max_frames][latent] f32 values
        float *rope = nullptr;   // [max_frames][head_dim] cos/sin by absolute position
        float *rvq_tail = nullptr;   // [2][hidden] RVQ rows of the last min(2, frames) frames, oldest first (pre_conv k3)
        float *halo_rows = nullptr;  // [halo][latent] output_proj rows of the last min(halo, frames) frames, oldest first
        // output stage (stream_set_output): the plain pushes refuse a stream that has one, the _out pushes need one
        bool has_out = false, out_final = false;   // out_final: a final push was made, no output push until a reset
        // an output push failed after the stream's frames were taken (frames / samples moved, the stage did not):
        // the next output push would filter samples that are gone, so the stream takes none until it is reset
        bool out_stale = false;
        int out_rate = 0, out_format = 0;
        int64_t out_samples = 0;     // output samples emitted so far = pcm_num_samples(samples, out_rate, out_final)
        float *out_hist = nullptr;   // [kPcmMaxHist] the stage's carried input history (its last K - 1 samples)
    };
    // look-back of the convolution stack in frames, derived from the loaded shapes (next to full_len)
    int stream_halo() const;
    // halo < 0: stream_halo(), or Q3T_VOC_STREAM_HALO when set (development knob); null + error when it does not fit
    Stream *stream_open(int max_frames, int halo = -1);
    // n_frames new frames of codes_host [n_frames][16] -> the next n_samples(P + n, 0) - n_samples(P, 0) samples.
    // Bad arguments (n_frames <= 0, more than max_frames in total, pcm_cap too small) fail before any state changes
    bool stream_push(Stream *st, const int32_t *codes_host, int n_frames, float *pcm_host, int64_t pcm_cap, int64_t *n_out);
    void stream_close(Stream *st);
    // back to zero frames and zero samples, keeping the caches: every carried row a push reads is bounded by the
    // frame count (cache rows [0, frames), min(2, frames) tail rows, min(halo, frames) halo rows), so nothing of the
    // previous utterance reaches the next one and the pushes after a reset are bit for bit a fresh stream's
    bool stream_reset(Stream *st);
    // One push on each of n_streams streams of this decoder (any mix of positions and sizes) through shared launches:
    // the row-wise stages run once over the packed new rows of all streams, the per-layer append and attention are one
    // launch each for all streams (voc_kv_append_batch / voc_attn_cached_batch), and pre_conv and the convolution
    // stack run once per group of streams with the same (n_frames, carried halo rows, carried tail rows), the group
    // as grid z.  pcm_host[j] receives stream j's samples, n_out[j] their count; they are, bit for bit, what
    // stream_push on stream j alone returns.  Every stream is validated before any state changes (a closed or foreign
    // stream, a duplicate, n_frames <= 0, more than max_frames in total, pcm_cap too small, a null pointer): on an
    // error no stream has moved and every n_out[j] is 0.
    bool stream_push_batch(int n_streams, Stream *const *sts, const int32_t *const *codes_host, const int32_t *n_frames,
                           float *const *pcm_host, const int64_t *pcm_cap, int64_t *n_out);
    // convolution-stack launch sequences (groups) of the last stream_push_batch; 0 after one that failed validation
    int stream_last_groups() const { return last_groups_; }

    // ---- output stage (pcm_out.h; DESIGN 2c "Output stage"): a decode's or a stream's f32 samples resampled to
    // spec.rate and written as spec.format on the device, so that only the client's bytes are copied back.
    struct OutSpec { int rate = 0, format = 0; };
    // The stage assumes the decoder's samples are at kPcmNativeRate (24000): the tokenizer GGUF carries no rate, every
    // shipped geometry runs at it, and q3t_get_config reports the same constant.
    bool check_spec(const OutSpec &spec);   // false + error naming the rate / format and listing the supported ones
    // one-shot decode (mode as decode()) through the stage with final = 1: *n_out samples of spec.format into out_host
    bool decode_out(const int32_t *codes_host, int n_frames, int mode, const OutSpec &spec, void *out_host,
                    int64_t out_cap_bytes, int64_t *n_out, int chunk_frames = 40);
    // only at zero frames (a fresh or reset stream); spec == nullptr clears it.  stream_reset keeps the spec and
    // rewinds the stage (history zeroed, counts 0)
    bool stream_set_output(Stream *st, const OutSpec *spec);
    // stream_push_batch through the stage: ONE pcm_out launch (plus the history update) after the launches of the
    // plain batched push, and device-to-host copies of the output bytes only.  Streams may carry different specs;
    // final[j] != 0 appends the filter's tail once and closes stream j's output until it is reset; such a push may
    // carry no frames (n_frames[j] == 0: the tail alone, no part in the vocoder's launches).  Stream j's bytes
    // are those of pushing it alone.  Validation and the error contract are stream_push_batch's, plus: a stream
    // without a spec, a stream already final, out_cap_bytes[j] smaller than the push's bytes
    bool stream_push_batch_out(int n_streams, Stream *const *sts, const int32_t *const *codes_host, const int32_t *n_frames,
                               const int32_t *final, void *const *out_host, const int64_t *out_cap_bytes, int64_t *n_out);

private:
    struct Conv { uint16_t *w = nullptr; float *b = nullptr; int k = 0, ic = 0, oc = 0; };   // w: [k][oc][ic]
    struct Snake { float *a = nullptr, *ib = nullptr; int n = 0; };                          // exp(alpha), exp(-beta)
    struct Layer {
        uint16_t *qkv = nullptr, *o = nullptr, *gu = nullptr, *down = nullptr;
        float *attn_norm = nullptr, *ffn_norm = nullptr, *attn_scale = nullptr, *ffn_scale = nullptr;
    };
    struct Up {
        Conv ct;
        uint16_t *dw = nullptr, *pw1 = nullptr, *pw2 = nullptr;
        float *dw_b = nullptr, *norm_w = nullptr, *norm_b = nullptr, *gamma = nullptr, *pw1_b = nullptr, *pw2_b = nullptr;
        int dw_k = 7, pw_dim = 0;
    };
    struct Res { Snake a1, a2; Conv c1, c2; int dil = 1; };
    struct Dec { Snake snake; Conv ct; Res res[3]; int rate = 1; };

    template <class T> T *dalloc(size_t n);
    int64_t full_len(int F) const;
    bool run_conv(const Conv &c, const float *x, int T, int pad, int dil, const Snake *sn, float *y, const float *resid,
                  int act, hipStream_t s);
    bool run_convT(const Conv &c, const float *x, int T, int stride, int trim, const Snake *sn, float *y, int T_out,
                   hipStream_t s);
    // the same convs on an f16 input already snake'd by the producer's epilogue; outputs f32 y and/or
    // y16 = f16(next_snake(y)) (the next conv's input), either may be null
    bool conv16(const Conv &c, const uint16_t *xh, int T, int pad, int dil, float *y, const float *resid, uint16_t *y16,
                const Snake *next, hipStream_t s);
    bool convT16(const Conv &c, const uint16_t *xh, int T, int stride, int trim, float *y, int T_out, uint16_t *y16,
                 const Snake *next, hipStream_t s);
    bool decode_rows(const int32_t *codes_dev, int F, float *pcm_dev, int64_t *n_out, hipStream_t s);
    // decode_rows' two halves.  frame_rows: RVQ .. output_proj of F frame rows per utterance into buf_[1] (a stream's
    // rows: against its state, written after the rows of its halo); conv_stack: upsample blocks .. output conv of the
    // T-frame sequences in buf_[1]
    bool frame_rows(const int32_t *codes_dev, int F, hipStream_t s, Stream *st);
    // frame_rows' row-wise parts, shared with stream_push_batch (packed rows of many streams)
    bool rvq_rows(const int32_t *codes_dev, int FR, float *out, hipStream_t s);
    bool layer_rows(const float *pre, int FR, float *out, hipStream_t s,
                    const std::function<bool(int, float *, uint16_t *)> &attn);
    bool conv_stack(int F, float *pcm_dev, int64_t *n_out, hipStream_t s);

    bool loaded_ = false;
    hipStream_t stream_ = nullptr;
    std::vector<void *> allocs_, scratch_;
    WeightArena wa_;   // every weight tensor (one blob)
    int n_usage_ = 0;
    int cb_dim_ = 0, cb_size_ = 0, hidden_ = 0, latent_ = 0, n_heads_ = 16, head_dim_ = 64, ffn_ = 0;
    uint16_t *cb_first_ = nullptr, *cb_rest_[15] = {}, *vq_first_out_ = nullptr, *vq_rest_out_ = nullptr;
    uint16_t *in_proj_ = nullptr, *out_proj_ = nullptr;
    float *in_proj_b_ = nullptr, *out_proj_b_ = nullptr, *pre_norm_ = nullptr;
    Conv pre_conv_, dec0_, dec6_;
    std::vector<Layer> layers_;
    Up up_[2];
    Dec dec_[4];
    Snake dec5_;
    // scratch (grown by ensure)
    int cap_frames_ = 0, batch_frames_ = 4096;
    size_t cap_big_ = 0, cap_ftot_ = 0, cap_pcm_ = 0;
    int nb_ = 1;   // utterances of the decode in flight (conv launches carry it as grid z)
    // the 96-channel residual units as one launch each (vocoder_resunit.hip); Q3T_VOC_FUSE=0: the two-conv form
    bool fuse_res_ = [] { const char *e = std::getenv("Q3T_VOC_FUSE"); return !(e && e[0] == '0'); }();
    float *buf_[3] = {nullptr, nullptr, nullptr};
    uint16_t *xh_ = nullptr;   // f16 (snake'd) conv input, one activation
    uint16_t *xh2_ = nullptr;  // second f16 activation: the decoder blocks ping-pong conv inputs written by epilogues
    int32_t *codes_ = nullptr;
    int *cols_ = nullptr;
    float *pcm_ = nullptr, *rope_ = nullptr;
    std::vector<Stream *> streams_;   // open streams (freed with the decoder)
    // stream_push_batch: the convolution-stack windows of every stream of a call, its device descriptors, group count
    float *sb_win_ = nullptr;
    void *sb_desc_ = nullptr;
    size_t sb_win_cap_ = 0, sb_desc_cap_ = 0;   // floats, bytes
    int last_groups_ = 0;
    // output stage: one request per stream of a batched push (null for the plain push), the per-rate tap tables (built
    // on first use), the f32 staging of a call's samples, its output bytes and its descriptors
    struct OutReq { const int32_t *final; void *const *out; const int64_t *cap; };
    bool push_batch(int n_streams, Stream *const *sts, const int32_t *const *codes_host, const int32_t *n_frames,
                    float *const *pcm_host, const int64_t *pcm_cap, int64_t *n_out, const OutReq *oreq);
    struct OutTaps { int rate = 0; PcmRate geo; float *taps = nullptr; };
    const OutTaps *out_taps(int rate);
    bool out_scratch(size_t stage_floats, size_t out_bytes, size_t n_desc);
    std::vector<OutTaps> out_taps_;
    float *po_stage_ = nullptr, *po_hist0_ = nullptr;
    unsigned char *po_bytes_ = nullptr;
    PcmOutDesc *po_desc_ = nullptr;
    size_t po_stage_cap_ = 0, po_bytes_cap_ = 0, po_desc_cap_ = 0;   // floats, bytes, descriptors
};

}  // namespace q3t
