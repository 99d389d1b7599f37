// vocoder.cpp — Qwen3-TTS tokenizer decoder on MI355X (see vocoder.h).  Restates, stage by stage,
// AudioTokenizerDecoder::build_graph (src/audio_tokenizer_decoder.cpp:622-802) with time-major activations.
#include "vocoder.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "vocoder_kernels.h"

namespace q3t {

Vocoder::~Vocoder() {
    while (!streams_.empty()) stream_close(streams_.back());
    for (void *p : allocs_) hipFree(p);
    for (void *p : scratch_) hipFree(p);
    if (sb_win_) hipFree(sb_win_);
    if (sb_desc_) hipFree(sb_desc_);
    for (const OutTaps &t : out_taps_) if (t.taps) hipFree(t.taps);
    for (void *p : {(void *)po_stage_, (void *)po_hist0_, (void *)po_bytes_, (void *)po_desc_}) if (p) hipFree(p);
}

template <class T>
T *Vocoder::dalloc(size_t n) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
    allocs_.push_back(p);
    return static_cast<T *>(p);
}

namespace {
const uint16_t *f16p(const GgufTensor *t) { return static_cast<const uint16_t *>(t->data); }
}  // namespace

bool Vocoder::load(const std::string &path, hipStream_t s, bool recv_weights) {
    stream_ = s;
    Gguf g;
    if (!g.open(path)) { set_error(g.error()); return false; }
    wa_.recv = recv_weights;
    const bool recv = recv_weights;   // shapes only: the tensor bytes are never read on receiving ranks
    size_t total = 0;
    for (const GgufTensor &t : g.tensors()) total += (t.nbytes() + 255) & ~(size_t)255;
    if (!wa_.reserve(total + ((size_t)1 << 20))) return false;
    auto T = [&](const std::string &n) -> const GgufTensor * {
        const GgufTensor *t = g.find(n);
        if (!t) set_error("missing vocoder tensor " + n);
        return t;
    };
    auto up16 = [&](const void *src, size_t n) -> uint16_t * {
        uint16_t *d = wa_.alloc<uint16_t>(n);
        if (d && !wa_.put(d, src, n * 2)) return nullptr;
        return d;
    };
    auto up32n = [&](const float *src, size_t n) -> float * {
        float *d = wa_.alloc<float>(n);
        if (d && !wa_.put(d, src, n * 4)) return nullptr;
        return d;
    };
    auto vec = [&](const std::string &n, int64_t expect) -> float * {
        const GgufTensor *t = T(n);
        if (!t) return nullptr;
        if (t->type != GGML_TYPE_F32 || (expect > 0 && t->nelements() != expect)) { set_error("bad f32 tensor " + n); return nullptr; }
        return up32n((const float *)t->data, (size_t)t->nelements());
    };
    // conv weight ne [K, C_in, C_out] (PyTorch [oc][ic][k]) -> per-tap [K][C_out][C_in]
    auto conv_w = [&](const std::string &n, Conv &c) -> bool {
        const GgufTensor *t = T(n);
        if (!t || t->type != GGML_TYPE_F16 || t->n_dims != 3) { set_error("bad conv " + n); return false; }
        c.k = (int)t->ne[0]; c.ic = (int)t->ne[1]; c.oc = (int)t->ne[2];
        const size_t nw = (size_t)c.k * c.oc * c.ic;
        std::vector<uint16_t> w(recv ? 0 : nw);
        const uint16_t *src = f16p(t);
        if (!recv)
            for (int oc = 0; oc < c.oc; ++oc)
                for (int ic = 0; ic < c.ic; ++ic)
                    for (int k = 0; k < c.k; ++k) w[((size_t)k * c.oc + oc) * c.ic + ic] = src[((size_t)oc * c.ic + ic) * c.k + k];
        c.w = up16(w.data(), nw);
        return c.w != nullptr;
    };
    // conv-transpose weight ne [K, C_out, C_in] (PyTorch [ic][oc][k]) -> per-tap [K][C_out][C_in]
    auto convT_w = [&](const std::string &n, Conv &c) -> bool {
        const GgufTensor *t = T(n);
        if (!t || t->type != GGML_TYPE_F16 || t->n_dims != 3) { set_error("bad conv_t " + n); return false; }
        c.k = (int)t->ne[0]; c.oc = (int)t->ne[1]; c.ic = (int)t->ne[2];
        const size_t nw = (size_t)c.k * c.oc * c.ic;
        std::vector<uint16_t> w(recv ? 0 : nw);
        const uint16_t *src = f16p(t);
        if (!recv)
            for (int ic = 0; ic < c.ic; ++ic)
                for (int oc = 0; oc < c.oc; ++oc)
                    for (int k = 0; k < c.k; ++k) w[((size_t)k * c.oc + oc) * c.ic + ic] = src[((size_t)ic * c.oc + oc) * c.k + k];
        c.w = up16(w.data(), nw);
        return c.w != nullptr;
    };
    auto mat = [&](const std::string &n, int &rows, int &cols) -> uint16_t * {
        const GgufTensor *t = T(n);
        if (!t || t->type != GGML_TYPE_F16) { set_error("bad matrix " + n); return nullptr; }
        cols = (int)(t->ne[0] == 1 && t->n_dims == 3 ? t->ne[1] : t->ne[0]);
        rows = (int)(t->nelements() / cols);
        return up16(t->data, (size_t)t->nelements());
    };
    // SnakeBeta: x + exp(-beta) * sin^2(exp(alpha) * x) (apply_snake, :375-402); exps precomputed once
    auto snake = [&](const std::string &pa, const std::string &pb, Snake &sn) -> bool {
        const GgufTensor *a = T(pa), *b = T(pb);
        if (!a || !b || a->type != GGML_TYPE_F32 || b->nelements() != a->nelements()) { set_error("bad snake " + pa); return false; }
        const size_t n = (size_t)a->nelements();
        std::vector<float> ea(recv ? 0 : n), ib(recv ? 0 : n);
        if (!recv)
            for (size_t i = 0; i < n; ++i) {
                ea[i] = expf(((const float *)a->data)[i]);
                ib[i] = expf(-((const float *)b->data)[i]);
            }
        sn.a = up32n(ea.data(), n);
        sn.ib = up32n(ib.data(), n);
        sn.n = (int)a->nelements();
        return sn.a && sn.ib;
    };

    // codebooks, divided by their usage counts when the file still carries them (normalize_codebooks,
    // src/audio_tokenizer_decoder.cpp:40-73: row r *= 1 / max(usage[r], 1e-5), re-rounded to f16).  The converter
    // already divides and drops *.usage (scripts/convert_tokenizer_to_gguf.py:347-359), so this is normally a no-op.
    auto codebook = [&](const std::string &name, const std::string &usage_name, uint16_t *&dst) -> bool {
        const GgufTensor *t = T(name);
        if (!t || t->type != GGML_TYPE_F16 || t->ne[0] != cb_dim_ || t->ne[1] != cb_size_) { set_error("bad codebook " + name); return false; }
        const GgufTensor *u = g.find(usage_name);
        if (!u) { dst = up16(t->data, (size_t)t->nelements()); return dst != nullptr; }
        if (u->type != GGML_TYPE_F32 || u->nelements() != cb_size_) { set_error("bad codebook usage " + usage_name); return false; }
        std::vector<uint16_t> w(recv ? 0 : (size_t)t->nelements());
        if (!recv) {
            const uint16_t *src = f16p(t);
            const float *us = static_cast<const float *>(u->data);
            for (int r = 0; r < cb_size_; ++r) {
                const float inv = 1.0f / std::max(us[r], 1e-5f);
                for (int d = 0; d < cb_dim_; ++d) {
                    const size_t i = (size_t)r * cb_dim_ + d;
                    _Float16 h;
                    std::memcpy(&h, src + i, 2);
                    const _Float16 o = (_Float16)((float)h * inv);   // round to nearest even
                    std::memcpy(&w[i], &o, 2);
                }
            }
        }
        dst = up16(w.data(), (size_t)t->nelements());
        ++n_usage_;
        return dst != nullptr;
    };
    const GgufTensor *cb = T("tok_dec.vq_first.0.codebook");
    if (!cb) return false;
    cb_dim_ = (int)cb->ne[0];
    cb_size_ = (int)cb->ne[1];
    if (!codebook("tok_dec.vq_first.0.codebook", "tok_dec.vq_first.0.usage", cb_first_)) return false;
    for (int i = 0; i < 15; ++i) {
        const std::string pre = "tok_dec.vq_rest." + std::to_string(i) + ".";
        if (!codebook(pre + "codebook", pre + "usage", cb_rest_[i])) return false;
    }
    int r, c;
    if (!(vq_first_out_ = mat("tok_dec.vq_first.output_proj.weight", r, c))) return false;
    hidden_ = r;
    if (c != cb_dim_) { set_error("vq output_proj shape"); return false; }
    if (!(vq_rest_out_ = mat("tok_dec.vq_rest.output_proj.weight", r, c))) return false;
    if (!conv_w("tok_dec.pre_conv.weight", pre_conv_)) return false;
    if (!(pre_conv_.b = vec("tok_dec.pre_conv.bias", pre_conv_.oc))) return false;
    latent_ = pre_conv_.oc;
    if (!(in_proj_ = mat("tok_dec.pre_tfm.input_proj.weight", r, c))) return false;
    if (!(in_proj_b_ = vec("tok_dec.pre_tfm.input_proj.bias", hidden_))) return false;
    n_heads_ = (int)g.get_int({"qwen3-tts-tokenizer.decoder.num_heads"}, 16);   // reference default 16
    head_dim_ = latent_ / n_heads_;
    for (int i = 0;; ++i) {
        const std::string p = "tok_dec.pre_tfm.blk." + std::to_string(i) + ".";
        if (!g.find(p + "attn_q.weight")) break;
        Layer L;
        std::vector<uint16_t> qkv;
        size_t n_qkv = 0;
        for (const char *nm : {"attn_q.weight", "attn_k.weight", "attn_v.weight"}) {
            const GgufTensor *t = T(p + nm);
            if (!t || t->ne[0] != hidden_ || t->ne[1] != latent_) { set_error("bad pre_tfm qkv"); return false; }
            if (!recv) qkv.insert(qkv.end(), f16p(t), f16p(t) + t->nelements());
            n_qkv += (size_t)t->nelements();
        }
        L.qkv = up16(qkv.data(), n_qkv);
        const GgufTensor *gt = T(p + "ffn_gate.weight"), *ut = T(p + "ffn_up.weight");
        if (!gt || !ut) return false;
        ffn_ = (int)gt->ne[1];
        if (ffn_ % 16) { set_error("pre_tfm ffn % 16"); return false; }
        const size_t n_gu = (size_t)2 * ffn_ * hidden_;
        std::vector<uint16_t> gu(recv ? 0 : n_gu);
        if (!recv)
            for (int blk = 0; blk < ffn_ / 16; ++blk) {
                std::memcpy(gu.data() + (size_t)(blk * 32) * hidden_, f16p(gt) + (size_t)(blk * 16) * hidden_, (size_t)16 * hidden_ * 2);
                std::memcpy(gu.data() + (size_t)(blk * 32 + 16) * hidden_, f16p(ut) + (size_t)(blk * 16) * hidden_, (size_t)16 * hidden_ * 2);
            }
        L.gu = up16(gu.data(), n_gu);
        if (!(L.o = mat(p + "attn_output.weight", r, c))) return false;
        if (!(L.down = mat(p + "ffn_down.weight", r, c))) return false;
        if (!(L.attn_norm = vec(p + "attn_norm.weight", hidden_)) || !(L.ffn_norm = vec(p + "ffn_norm.weight", hidden_)) ||
            !(L.attn_scale = vec(p + "attn_scale", hidden_)) || !(L.ffn_scale = vec(p + "ffn_scale", hidden_)))
            return false;
        layers_.push_back(L);
    }
    if (!(pre_norm_ = vec("tok_dec.pre_tfm.norm.weight", hidden_))) return false;
    if (!(out_proj_ = mat("tok_dec.pre_tfm.output_proj.weight", r, c))) return false;
    if (!(out_proj_b_ = vec("tok_dec.pre_tfm.output_proj.bias", latent_))) return false;
    for (int u = 0; u < 2; ++u) {
        const std::string p = "tok_dec.upsample." + std::to_string(u) + ".";
        Up &U = up_[u];
        if (!convT_w(p + "conv.weight", U.ct)) return false;
        if (!(U.ct.b = vec(p + "conv.bias", U.ct.oc))) return false;
        const GgufTensor *dw = T(p + "dwconv.weight");
        if (!dw || dw->ne[1] != 1) { set_error("bad dwconv"); return false; }
        U.dw_k = (int)dw->ne[0];
        U.dw = up16(dw->data, (size_t)dw->nelements());
        if (!(U.dw_b = vec(p + "dwconv.bias", U.ct.oc)) || !(U.norm_w = vec(p + "norm.weight", U.ct.oc)) ||
            !(U.norm_b = vec(p + "norm.bias", U.ct.oc)) || !(U.gamma = vec(p + "gamma", U.ct.oc)))
            return false;
        if (!(U.pw1 = mat(p + "pwconv1.weight", U.pw_dim, c))) return false;
        if (!(U.pw1_b = vec(p + "pwconv1.bias", U.pw_dim))) return false;
        if (!(U.pw2 = mat(p + "pwconv2.weight", r, c))) return false;
        if (!(U.pw2_b = vec(p + "pwconv2.bias", U.ct.oc))) return false;
    }
    if (!conv_w("tok_dec.dec.0.conv.weight", dec0_)) return false;
    if (!(dec0_.b = vec("tok_dec.dec.0.conv.bias", dec0_.oc))) return false;
    const int rates[4] = {8, 5, 4, 3};   // audio_tokenizer_decoder.cpp:766
    for (int d = 0; d < 4; ++d) {
        const std::string p = "tok_dec.dec." + std::to_string(d + 1) + ".";
        Dec &D = dec_[d];
        D.rate = rates[d];
        if (!snake(p + "snake.alpha", p + "snake.beta", D.snake)) return false;
        if (!convT_w(p + "conv_t.weight", D.ct)) return false;
        if (!(D.ct.b = vec(p + "conv_t.bias", D.ct.oc))) return false;
        if (D.ct.k > 2 * D.rate || D.ct.k < D.rate) { set_error("unsupported conv_t kernel size"); return false; }
        for (int ri = 0; ri < 3; ++ri) {
            const std::string q = p + "res." + std::to_string(ri + 2) + ".";
            Res &R = D.res[ri];
            R.dil = ri == 0 ? 1 : ri == 1 ? 3 : 9;   // :324-328
            if (!snake(q + "act1.alpha", q + "act1.beta", R.a1) || !snake(q + "act2.alpha", q + "act2.beta", R.a2)) return false;
            if (!conv_w(q + "conv1.weight", R.c1) || !conv_w(q + "conv2.weight", R.c2)) return false;
            if (!(R.c1.b = vec(q + "conv1.bias", R.c1.oc)) || !(R.c2.b = vec(q + "conv2.bias", R.c2.oc))) return false;
        }
    }
    if (!snake("tok_dec.dec.5.snake.alpha", "tok_dec.dec.5.snake.beta", dec5_)) return false;
    if (!conv_w("tok_dec.dec.6.conv.weight", dec6_)) return false;
    if (!(dec6_.b = vec("tok_dec.dec.6.conv.bias", dec6_.oc))) return false;
    if (head_dim_ != 64) { set_error("vocoder head_dim must be 64"); return false; }
    loaded_ = true;
    return true;
}

int64_t Vocoder::full_len(int F) const {
    if (F <= 0) return 0;
    int64_t T = F;
    for (int u = 0; u < 2; ++u) T = (T - 1) * 2 + up_[u].ct.k;
    for (int d = 0; d < 4; ++d) { const int s = dec_[d].rate, K = dec_[d].ct.k; T = (T - 1) * s + K - 2 * (K - s); }
    return T;
}
// Frames of left context the convolution stack needs to reproduce the samples of a push (DESIGN 2c "Vocoder
// stream").  full_len is affine in F, rate * F - lead: a push at frame boundary P starts `lead` samples before that
// boundary.  L is how far before the boundary, in steps of the current stage, the stage's output is still read; walk
// the stack from the PCM back to the frame rows: a causal conv (k, dilation d) reads (k-1)*d steps back; a transposed
// conv of stride s whose output t, after trimming `trim` on the left, gathers inputs ceil((t + trim - K + 1) / s) ..
// floor((t + trim) / s) maps L steps back to floor((L + K - 1 - trim) / s) input steps back (with trim = K - s that is
// ceil(L / s): the second input step a K = 2s kernel reads lies ahead of t, not behind it).
int Vocoder::stream_halo() const {
    if (!loaded_) return 0;
    const int64_t rate = full_len(2) - full_len(1), lead = rate - full_len(1);
    int64_t L = std::max<int64_t>(lead, 0);
    L += dec6_.k - 1;
    for (int d = 3; d >= 0; --d) {
        const Dec &D = dec_[d];
        for (int ri = 2; ri >= 0; --ri) L += (int64_t)(D.res[ri].c1.k - 1) * D.res[ri].dil + (D.res[ri].c2.k - 1);
        const int s = D.rate, K = D.ct.k, trim = K - s;
        L = (L + K - 1 - trim) / s;
    }
    L += dec0_.k - 1;
    for (int u = 1; u >= 0; --u) {
        L += up_[u].dw_k - 1;
        L = (L + up_[u].ct.k - 1) / 2;   // stride 2, no trimming
    }
    return (int)L;
}

double Vocoder::decode_flops(int F) const {
    if (F <= 0 || !loaded_) return 0.0;
    const double f = F, VH = hidden_, LAT = latent_;
    auto conv = [](double T_out, const Conv &c) { return 2.0 * T_out * c.ic * c.oc * c.k; };
    double fl = 16.0 * 2.0 * f * cb_dim_ * VH;                 // RVQ output projections
    fl += conv(f, pre_conv_) + 2.0 * f * LAT * VH;             // pre-conv, input_proj
    for (size_t l = 0; l < layers_.size(); ++l)
        fl += 2.0 * f * VH * 3 * LAT + 2.0 * 2.0 * (f * (f + 1) / 2) * LAT + 2.0 * f * LAT * VH +
              2.0 * f * VH * 2 * ffn_ + 2.0 * f * ffn_ * VH;
    fl += 2.0 * f * VH * LAT;                                  // output_proj
    double T = f;
    for (int u = 0; u < 2; ++u) {
        const double T1 = (T - 1) * 2 + up_[u].ct.k;
        fl += conv(T, up_[u].ct) + 2.0 * T1 * LAT * up_[u].dw_k + 2.0 * 2.0 * T1 * LAT * up_[u].pw_dim;
        T = T1;
    }
    fl += conv(T, dec0_);
    for (int d = 0; d < 4; ++d) {
        const Dec &D = dec_[d];
        const double T2 = (T - 1) * D.rate + D.ct.k - 2 * (D.ct.k - D.rate);
        fl += conv(T, D.ct);   // every input row meets every tap once (before trimming)
        for (int r = 0; r < 3; ++r) fl += conv(T2, D.res[r].c1) + conv(T2, D.res[r].c2);
        T = T2;
    }
    return fl + conv(T, dec6_);
}

int64_t Vocoder::n_samples(int n_frames, int mode) const {
    if (n_frames <= 0) return 0;
    return mode == 0 ? full_len(n_frames) : (int64_t)n_frames * 1920;
}

// scratch for nb utterances of F frames: sized by the totals (largest activation x nb, frames x nb), so a batch of
// short utterances reuses the scratch of one long one
// rows: packed frame rows of a row-wise pass that belong to no single sequence (a batched stream push)
bool Vocoder::ensure(int F, int nb, size_t rows) {
    size_t big = 0;   // largest [T][C] activation of one utterance over the stages
    int64_t T = F;
    big = std::max(big, (size_t)F * std::max(latent_, 3 * latent_));
    for (int u = 0; u < 2; ++u) { T = (T - 1) * 2 + up_[u].ct.k; big = std::max(big, (size_t)T * up_[u].pw_dim / 2 + (size_t)T * latent_); }
    big = std::max(big, (size_t)T * dec0_.oc);
    for (int d = 0; d < 4; ++d) {
        const int s = dec_[d].rate, K = dec_[d].ct.k;
        T = (T - 1) * s + K - 2 * (K - s);
        big = std::max(big, (size_t)T * dec_[d].ct.oc);
    }
    big *= (size_t)nb;
    // per packed row: qkv, an RVQ row, or the attention output and the FFN's hidden row in f16
    big = std::max(big, rows * (size_t)std::max({3 * latent_, hidden_, (latent_ + ffn_ + 1) / 2}));
    const size_t frames = std::max((size_t)F * nb, rows);
    const size_t pcm = (size_t)nb * std::max<int64_t>(full_len(F), (int64_t)F * 1920);
    if (big <= cap_big_ && frames <= cap_ftot_ && pcm <= cap_pcm_ && F <= cap_frames_) return true;
    big = std::max(big, cap_big_);
    const size_t fr = std::max(frames, cap_ftot_), pc = std::max(pcm, cap_pcm_);
    F = std::max(F, cap_frames_);
    for (void *p : scratch_) hipFree(p);
    scratch_.clear();
    cap_big_ = cap_ftot_ = cap_pcm_ = 0;
    cap_frames_ = 0;
    auto alloc = [&](size_t bytes) -> void * {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        scratch_.push_back(p);
        return p;
    };
    for (int i = 0; i < 3; ++i) if (!(buf_[i] = (float *)alloc(big * 4))) { set_error("vocoder scratch alloc"); return false; }
    if (!(xh_ = (uint16_t *)alloc(big * 2)) || !(xh2_ = (uint16_t *)alloc(big * 2))) { set_error("vocoder scratch alloc"); return false; }
    codes_ = (int32_t *)alloc(fr * 16 * 4);
    cols_ = (int *)alloc(fr * 16 * 4);
    pcm_ = (float *)alloc(pc * 4);
    // RoPE cos/sin table (theta 1e4, head_dim 64) with the ggml_rope_cache_init recurrence
    std::vector<float> rope((size_t)F * head_dim_);
    const float theta_scale = powf(10000.0f, -2.0f / (float)head_dim_);
    for (int p = 0; p < F; ++p) {
        float theta = (float)p;
        for (int i0 = 0; i0 < head_dim_; i0 += 2) {
            rope[(size_t)p * head_dim_ + i0] = cosf(theta);
            rope[(size_t)p * head_dim_ + i0 + 1] = sinf(theta);
            theta *= theta_scale;
        }
    }
    rope_ = (float *)alloc(rope.size() * 4);
    if (!codes_ || !cols_ || !pcm_ || !rope_) { set_error("vocoder scratch alloc"); return false; }
    Q3T_HIP(hipMemcpy(rope_, rope.data(), rope.size() * 4, hipMemcpyHostToDevice));
    cap_big_ = big; cap_ftot_ = fr; cap_pcm_ = pc;
    cap_frames_ = F;
    return true;
}

// causal conv (ggml_pad_ext left + ggml_conv_1d, stride 1) as one implicit-GEMM launch
bool Vocoder::run_conv(const Conv &c, const float *x, int T, int pad, int dil, const Snake *sn, float *y,
                       const float *resid, int act, hipStream_t s) {
    ConvParams p;
    p.x = x; p.T_in = T; p.C_in = c.ic;
    if (c.ic % 8 == 0) {   // SnakeBeta + f16 rounding once per element, not once per output tile and tap window
        if (!snake_f16(x, sn ? sn->a : nullptr, sn ? sn->ib : nullptr, xh_, (int64_t)T * nb_, c.ic, s)) return false;
        p.xh = xh_;
    } else if (sn) {
        p.snake_a = sn->a; p.snake_ib = sn->ib;
    }
    p.n_taps = c.k;
    for (int j = 0; j < c.k; ++j) p.taps[j] = ConvTap{c.w + (size_t)j * c.oc * c.ic, j * dil - pad};
    p.dmin = -pad; p.dmax = (c.k - 1) * dil - pad;
    p.y = y; p.C_out = c.oc; p.M = T + pad - dil * (c.k - 1); p.so = 1; p.ob = 0;
    p.bias = c.b; p.resid = resid; p.act = act;
    p.nb = nb_; p.xbs = T; p.ybs = p.M;
    return conv(p, s);
}

// ggml_conv_transpose_1d (stride st, no padding) followed by trimming `trim` samples on both sides, + bias,
// decomposed into st output phases: output t = st*m + phi gathers taps k = k0 + j*st with input row m + dj.
bool Vocoder::run_convT(const Conv &c, const float *x, int T, int st, int trim, const Snake *sn, float *y, int T_out,
                        hipStream_t s) {
    const bool pre = c.ic % 8 == 0;   // one snake/f16 pass shared by the st output phases
    if (pre && !snake_f16(x, sn ? sn->a : nullptr, sn ? sn->ib : nullptr, xh_, (int64_t)T * nb_, c.ic, s)) return false;
    for (int phi = 0; phi < st; ++phi) {
        ConvParams p;
        p.x = x; p.T_in = T; p.C_in = c.ic;
        if (pre) p.xh = xh_;
        else if (sn) { p.snake_a = sn->a; p.snake_ib = sn->ib; }
        const int k0 = (phi + trim) % st;
        int n = 0, dmin = 1 << 30, dmax = -(1 << 30);
        for (int k = k0; k < c.k; k += st) {
            const int dj = (phi + trim - k) / st;   // exact: (phi + trim - k) divisible by st
            p.taps[n++] = ConvTap{c.w + (size_t)k * c.oc * c.ic, dj};
            dmin = std::min(dmin, dj);
            dmax = std::max(dmax, dj);
        }
        if (n == 0) continue;
        p.n_taps = n; p.dmin = dmin; p.dmax = dmax;
        p.y = y; p.C_out = c.oc; p.M = (T_out - phi + st - 1) / st; p.so = st; p.ob = phi;
        p.bias = c.b;
        p.nb = nb_; p.xbs = T; p.ybs = T_out;
        if (!conv(p, s)) return false;
    }
    return true;
}

bool Vocoder::conv16(const Conv &c, const uint16_t *xh, int T, int pad, int dil, float *y, const float *resid,
                     uint16_t *y16, const Snake *next, hipStream_t s) {
    ConvParams p;
    p.xh = xh; p.T_in = T; p.C_in = c.ic;
    p.n_taps = c.k;
    for (int j = 0; j < c.k; ++j) p.taps[j] = ConvTap{c.w + (size_t)j * c.oc * c.ic, j * dil - pad};
    p.dmin = -pad; p.dmax = (c.k - 1) * dil - pad;
    p.y = y; p.C_out = c.oc; p.M = T + pad - dil * (c.k - 1); p.so = 1; p.ob = 0;
    p.bias = c.b; p.resid = resid;
    p.y16 = y16;
    if (next) { p.y16_a = next->a; p.y16_ib = next->ib; }
    p.nb = nb_; p.xbs = T; p.ybs = p.M;
    return conv(p, s);
}

bool Vocoder::convT16(const Conv &c, const uint16_t *xh, int T, int st, int trim, float *y, int T_out, uint16_t *y16,
                      const Snake *next, hipStream_t s) {
    if (c.ic % 32 == 0 && (c.oc % 96 == 0 || c.oc % 64 == 0) && c.k <= st * CONV_MAX_TAPS) {
        // every output phase in one launch (grid z)
        ConvParams p;
        p.xh = xh; p.T_in = T; p.C_in = c.ic;
        p.ct_w = c.w; p.ct_k = c.k; p.ct_st = st; p.ct_trim = trim; p.T_out = T_out;
        p.y = y; p.C_out = c.oc; p.bias = c.b; p.y16 = y16;
        if (next) { p.y16_a = next->a; p.y16_ib = next->ib; }
        p.nb = nb_; p.xbs = T; p.ybs = T_out;
        return conv(p, s);
    }
    for (int phi = 0; phi < st; ++phi) {
        ConvParams p;
        p.xh = xh; p.T_in = T; p.C_in = c.ic;
        const int k0 = (phi + trim) % st;
        int n = 0, dmin = 1 << 30, dmax = -(1 << 30);
        for (int k = k0; k < c.k; k += st) {
            const int dj = (phi + trim - k) / st;
            p.taps[n++] = ConvTap{c.w + (size_t)k * c.oc * c.ic, dj};
            dmin = std::min(dmin, dj);
            dmax = std::max(dmax, dj);
        }
        if (n == 0) continue;
        p.n_taps = n; p.dmin = dmin; p.dmax = dmax;
        p.y = y; p.C_out = c.oc; p.M = (T_out - phi + st - 1) / st; p.so = st; p.ob = phi;
        p.bias = c.b;
        p.y16 = y16;
        if (next) { p.y16_a = next->a; p.y16_ib = next->ib; }
        p.nb = nb_; p.xbs = T; p.ybs = T_out;
        if (!conv(p, s)) return false;
    }
    return true;
}

bool Vocoder::decode_device(const int32_t *codes_dev, int F, float *pcm_dev, int64_t *n_out, hipStream_t s, int nb) {
    if (nb < 1 || F > cap_frames_ || (size_t)F * nb > cap_ftot_) { set_error("vocoder: decode larger than ensure()"); return false; }
    nb_ = nb;
    const bool ok = decode_rows(codes_dev, F, pcm_dev, n_out, s);
    nb_ = 1;
    return ok;
}

// the row GEMVs of a decode: kernel family and K split pinned to one batch size, so a row's arithmetic does not depend
// on how many frame rows the launch covers (an utterance decoded alone, or padded into a batch, gives the same bits)
static GemvParams row_gemv() {
    GemvParams g;
    g.family_b = 64;
    return g;
}

// one decode of nb_ utterances of F frames: row-wise stages (RVQ, projections, norms, 1-tap convs) run over all
// nb_*F rows, sequence stages (causal convs, transposed convs, attention) carry the utterance as grid z
bool Vocoder::decode_rows(const int32_t *codes_dev, int F, float *pcm_dev, int64_t *n_out, hipStream_t s) {
    return frame_rows(codes_dev, F, s, nullptr) && conv_stack(F, pcm_dev, n_out, s);
}

// RVQ of FR packed frame rows: latent = W_first . cb_first[c0] + sum_k W_rest . cb_rest_k[c_{k+1}]   (:650-703) -> out
// [FR][hidden]; buf_[1] holds the running sum (out may be any other buffer)
bool Vocoder::rvq_rows(const int32_t *codes_dev, int FR, float *out, hipStream_t s) {
    const int VH = hidden_;
    float *B = buf_[1];
    if (!codes_cols(codes_dev, cols_, FR, 16, s)) return false;
    GemvParams g = row_gemv();
    g.N = VH; g.K = cb_dim_; g.B = FR; g.pro = PRO_F16; g.ldx = cb_dim_; g.ldo = VH;
    for (int k = 0; k < 15; ++k) {
        g.W = vq_rest_out_; g.x = cb_rest_[k]; g.x_idx = cols_ + (size_t)(k + 1) * FR;
        g.resid = k == 0 ? nullptr : B; g.ldr = VH; g.out_f32 = B;
        if (!gemv(g, s)) return false;
    }
    g.W = vq_first_out_; g.x = cb_first_; g.x_idx = cols_; g.resid = nullptr; g.aux = B; g.lda = VH;
    g.out_f32 = out;
    return gemv(g, s);
}

// input_proj .. output_proj of FR packed frame rows: pre [FR][latent] (pre_conv's rows) -> out [FR][latent].  x lives
// in buf_[0], qkv in buf_[1], the attention output and the FFN's hidden rows in buf_[2]; attn(layer, qkv, att) runs the
// layer's attention (RoPE included) from qkv [FR][3*latent] into att [FR][latent] f16.  out may be in buf_[1] or buf_[2]
bool Vocoder::layer_rows(const float *pre, int FR, float *out, hipStream_t s,
                         const std::function<bool(int, float *, uint16_t *)> &attn) {
    const int VH = hidden_, LAT = latent_;
    float *A = buf_[0], *B = buf_[1], *C = buf_[2];
    // 3) input_proj + bias -> x [F][VH]
    GemvParams ip = row_gemv();
    ip.W = in_proj_; ip.N = VH; ip.K = LAT; ip.B = FR; ip.pro = PRO_F32; ip.x = pre; ip.ldx = LAT;
    ip.bias = in_proj_b_; ip.out_f32 = A; ip.ldo = VH;
    if (!gemv(ip, s)) return false;
    float *x = A;
    float *qkv = B;                                        // [F][3*LAT]
    uint16_t *att = reinterpret_cast<uint16_t *>(C);       // [F][LAT] f16
    uint16_t *hm = reinterpret_cast<uint16_t *>(C) + (size_t)FR * LAT;   // [F][ffn] f16
    // large-M projections (M = frames or upsampled steps) run as 1-tap convs on the implicit-GEMM conv kernel over
    // pre-normalised f16 rows (norm_f16 reproduces the GEMM prologue's norm); the decode-shaped GEMM path stays for
    // the shapes the conv tiles do not cover
    const bool qkv_conv = VH % 32 == 0 && VH <= 1024 && VH % 4 == 0 && (3 * LAT) % 96 == 0;
    for (const Layer &L : layers_) {
        if (qkv_conv) {
            if (!norm_f16(x, L.attn_norm, nullptr, 1e-5f, 0, xh_, FR, VH, s)) return false;
            ConvParams q;
            q.xh = xh_; q.T_in = FR; q.C_in = VH; q.n_taps = 1; q.taps[0] = ConvTap{L.qkv, 0};
            q.y = qkv; q.C_out = 3 * LAT; q.M = FR;
            if (!conv(q, s)) return false;
        } else {
            GemvParams q = row_gemv();
            q.W = L.qkv; q.N = 3 * LAT; q.K = VH; q.B = FR; q.pro = PRO_RMS; q.x = x; q.ldx = VH; q.nw = L.attn_norm;
            q.eps = 1e-5f; q.out_f32 = qkv; q.ldo = 3 * LAT;
            if (!gemv(q, s)) return false;
        }
        if (!attn((int)(&L - layers_.data()), qkv, att)) return false;
        GemvParams o = row_gemv();
        o.W = L.o; o.N = VH; o.K = LAT; o.B = FR; o.pro = PRO_F16; o.x = att; o.ldx = LAT;
        o.scale = L.attn_scale; o.resid = x; o.ldr = VH; o.out_f32 = x; o.ldo = VH;
        if (!gemv(o, s)) return false;
        GemvParams gu = row_gemv();
        gu.W = L.gu; gu.N = 2 * ffn_; gu.K = VH; gu.B = FR; gu.pro = PRO_RMS; gu.x = x; gu.ldx = VH; gu.nw = L.ffn_norm;
        gu.eps = 1e-5f; gu.act = ACT_SWIGLU; gu.out_f16 = hm; gu.ldo = ffn_;
        if (!gemv(gu, s)) return false;
        GemvParams dn = row_gemv();
        dn.W = L.down; dn.N = VH; dn.K = ffn_; dn.B = FR; dn.pro = PRO_F16; dn.x = hm; dn.ldx = ffn_;
        dn.scale = L.ffn_scale; dn.resid = x; dn.ldr = VH; dn.out_f32 = x; dn.ldo = VH;
        if (!gemv(dn, s)) return false;
    }
    // final RMSNorm + output_proj + bias -> [F][LAT]   (:740-744)
    GemvParams op = row_gemv();
    op.W = out_proj_; op.N = LAT; op.K = VH; op.B = FR; op.pro = PRO_RMS; op.x = x; op.ldx = VH; op.nw = pre_norm_;
    op.eps = 1e-5f; op.bias = out_proj_b_; op.out_f32 = out; op.ldo = LAT;
    return gemv(op, s);
}

// Frame-rate half.  st null: the whole utterances of a one-shot decode.  st set (nb_ = 1): the F new frames of a stream
// at positions P..P+F-1 -- pre_conv sees the RVQ rows of the previous two frames in front of the new ones, the
// attention runs against the stream's K/V caches, and output_proj's rows land after the stream's halo rows in buf_[1],
// which then holds the window the convolution stack runs on.  Every launch is the one-shot path's on fewer rows.
bool Vocoder::frame_rows(const int32_t *codes_dev, int F, hipStream_t s, Stream *st) {
    const int VH = hidden_, LAT = latent_;
    const int FR = F * nb_;   // frame rows of the batch
    float *A = buf_[0], *B = buf_[1], *C = buf_[2];
    const int P = st ? st->frames : 0;
    const int tail = st ? std::min(2, P) : 0;            // carried RVQ rows in front of the new ones
    const int hrows = st ? std::min(st->halo, P) : 0;    // carried output_proj rows in front of the new ones
    // 1) RVQ
    if (!rvq_rows(codes_dev, FR, A + (size_t)tail * VH, s)) return false;
    if (st) {
        if (tail) Q3T_HIP(hipMemcpyAsync(A, st->rvq_tail, (size_t)tail * VH * 4, hipMemcpyDeviceToDevice, s));
        const int keep = std::min(2, P + F);   // the next push's tail: the last rows of [tail + F]
        Q3T_HIP(hipMemcpyAsync(st->rvq_tail, A + (size_t)(tail + F - keep) * VH, (size_t)keep * VH * 4,
                               hipMemcpyDeviceToDevice, s));
    }
    // 2) causal pre-conv k3 (left pad 2) -> [F][LAT]   (:705-718)
    if (!run_conv(pre_conv_, A, tail + F, 2, 1, nullptr, C, nullptr, 0, s)) return false;
    // 3) the transformer over the new rows
    auto attn = [&](int layer, float *qkv, uint16_t *att) {
        if (!st) return attn_prefill(qkv, rope_, att, F, n_heads_, head_dim_, s, nb_);
        const size_t lo = (size_t)layer * st->max_frames * LAT;   // this layer's cache
        return voc_kv_append(qkv, st->rope, st->kc + lo, st->vc + lo, P, F, n_heads_, head_dim_, s) &&
               voc_attn_cached(qkv, st->kc + lo, st->vc + lo, att, P, F, n_heads_, head_dim_, s);
    };
    if (!layer_rows(C + (size_t)tail * LAT, FR, B + (size_t)hrows * LAT, s, attn)) return false;
    if (st) {
        if (hrows) Q3T_HIP(hipMemcpyAsync(B, st->halo_rows, (size_t)hrows * LAT * 4, hipMemcpyDeviceToDevice, s));
        const int keep = std::min(st->halo, P + F);   // the next push's halo: the last rows of [hrows + F]
        if (keep)
            Q3T_HIP(hipMemcpyAsync(st->halo_rows, B + (size_t)(hrows + F - keep) * LAT, (size_t)keep * LAT * 4,
                                   hipMemcpyDeviceToDevice, s));
    }
    return true;
}

// Convolution half: the nb_ sequences of F frame rows [F][LAT] in buf_[1] -> PCM
bool Vocoder::conv_stack(int F, float *pcm_dev, int64_t *n_out, hipStream_t s) {
    const int LAT = latent_;
    float *A = buf_[0], *B = buf_[1], *C = buf_[2];
    float *cur = B;
    float *f0 = A, *f1 = C;
    int64_t T = F;
    // 4) ConvNeXt upsample blocks (:490-549)
    for (int u = 0; u < 2; ++u) {
        const Up &U = up_[u];
        const int64_t T1 = (T - 1) * 2 + U.ct.k;
        float *h = f0;                                   // conv-transpose output = residual [T1][LAT]
        if (!run_convT(U.ct, cur, (int)T, 2, 0, nullptr, h, (int)T1, s)) return false;
        float *dwo = f1;                                 // [T1][LAT]
        if (!dwconv(h, U.dw, U.dw_b, dwo, (int)T1, LAT, U.dw_k, s, nb_)) return false;
        uint16_t *pw = reinterpret_cast<uint16_t *>(cur);  // [T1][pw_dim] f16, cur is dead now (ensure() sizes it)
        const bool pw_conv = LAT % 32 == 0 && LAT <= 1024 && U.pw_dim % 64 == 0 && U.pw_dim % 32 == 0 && LAT % 64 == 0;
        if (pw_conv) {
            // LayerNorm -> f16 rows, pw1 + bias + GELU -> f16, pw2 + bias, x gamma, + residual (in place)
            if (!norm_f16(dwo, U.norm_w, U.norm_b, 1e-6f, 1, xh_, (int)T1 * nb_, LAT, s)) return false;
            ConvParams c1;
            c1.xh = xh_; c1.T_in = (int)T1 * nb_; c1.C_in = LAT; c1.n_taps = 1; c1.taps[0] = ConvTap{U.pw1, 0};
            c1.C_out = U.pw_dim; c1.M = (int)T1 * nb_; c1.bias = U.pw1_b; c1.act = 4; c1.y16 = pw;
            if (!conv(c1, s)) return false;
            ConvParams c2;
            c2.xh = pw; c2.T_in = (int)T1 * nb_; c2.C_in = U.pw_dim; c2.n_taps = 1; c2.taps[0] = ConvTap{U.pw2, 0};
            c2.C_out = LAT; c2.M = (int)T1 * nb_; c2.bias = U.pw2_b; c2.scale = U.gamma; c2.resid = h; c2.y = h;
            if (!conv(c2, s)) return false;
        } else {
            GemvParams p1 = row_gemv();
            p1.W = U.pw1; p1.N = U.pw_dim; p1.K = LAT; p1.B = (int)T1 * nb_; p1.pro = PRO_LN; p1.x = dwo; p1.ldx = LAT;
            p1.nw = U.norm_w; p1.nb = U.norm_b; p1.eps = 1e-6f; p1.bias = U.pw1_b; p1.act = ACT_GELU;
            p1.out_f16 = pw; p1.ldo = U.pw_dim;
            if (!gemv(p1, s)) return false;
            GemvParams p2 = row_gemv();
            p2.W = U.pw2; p2.N = LAT; p2.K = U.pw_dim; p2.B = (int)T1 * nb_; p2.pro = PRO_F16; p2.x = pw; p2.ldx = U.pw_dim;
            p2.bias = U.pw2_b; p2.scale = U.gamma; p2.resid = h; p2.ldr = LAT; p2.out_f32 = h; p2.ldo = LAT;
            if (!gemv(p2, s)) return false;
        }
        float *nxt = h;
        f0 = cur; cur = nxt; T = T1;
    }
    // 5) dec0 conv k7 (left pad 6) -> [T][dec_dim]   (:759-763).  From here on every conv input is the f16
    // SnakeBeta of its predecessor's output, written by that conv's epilogue (snake + rounding once per element,
    // the f32 tensor itself only where a residual needs it): ha / hb ping-pong
    uint16_t *ha = xh_, *hb = xh2_;
    if (!snake_f16(cur, nullptr, nullptr, ha, T * nb_, dec0_.ic, s)) return false;
    if (!conv16(dec0_, ha, (int)T, 6, 1, nullptr, nullptr, hb, &dec_[0].snake, s)) return false;   // snake(dec0) only
    std::swap(ha, hb);
    // 6) decoder blocks: SnakeBeta -> conv-transpose (trim K-s both sides) + bias -> 3 residual units (:551-620)
    for (int d = 0; d < 4; ++d) {
        const Dec &D = dec_[d];
        const int st = D.rate, K = D.ct.k;
        const int64_t T2 = (T - 1) * st + K - 2 * (K - st);
        // x = convT(snake(x)): f32 residual stream + f16 snake1 of residual unit 0
        if (!convT16(D.ct, ha, (int)T, st, K - st, f0, (int)T2, hb, &D.res[0].a1, s)) return false;
        std::swap(ha, hb);
        std::swap(cur, f0);
        T = T2;
        for (int ri = 0; ri < 3; ++ri) {
            const Res &R = D.res[ri];
            const Snake *next = ri < 2 ? &D.res[ri + 1].a1 : d < 3 ? &dec_[d + 1].snake : &dec5_;
            // the last unit of the last block feeds only the output conv's f16 input: no f32 residual stream out
            float *xout = d == 3 && ri == 2 ? nullptr : cur;
            if (fuse_res_ && R.c1.ic == 96 && R.c1.oc == 96 && R.c1.k == 7 && R.c2.ic == 96 && R.c2.oc == 96 && R.c2.k == 1 &&
                R.dil <= 9 && R.c1.b && R.c2.b) {
                // the whole unit in one launch (vocoder_resunit.hip): h stays on chip, bit-identical to the two convs
                ResUnitParams u;
                u.xh = ha; u.x = cur; u.y = xout; u.y16 = hb; u.T = (int)T; u.dil = R.dil;
                u.w1 = R.c1.w; u.b1 = R.c1.b; u.a2 = R.a2.a; u.ib2 = R.a2.ib;
                u.w2 = R.c2.w; u.b2 = R.c2.b; u.an = next->a; u.ibn = next->ib;
                u.nb = nb_; u.bs = T;
                if (!resunit96(u, s)) return false;
                std::swap(ha, hb);
                continue;
            }
            // h1 = conv1(snake1(x)) with causal pad 6*dil -> only snake2(h1) in f16; x += conv2(snake2(h1)) (f32, in
            // place) plus the next conv's f16 input
            if (!conv16(R.c1, ha, (int)T, 6 * R.dil, R.dil, nullptr, nullptr, hb, &R.a2, s)) return false;
            if (!conv16(R.c2, hb, (int)T, 0, 1, xout, cur, ha, next, s)) return false;
        }
    }
    // 7) SnakeBeta -> conv k7 (pad 6) -> tanh   (:775-790): ha holds f16(snake(dec5)) of the stream
    if (dec6_.oc == 1 && dec6_.ic % 8 == 0 && dec6_.ic <= 104 && dec6_.k <= 8) {
        if (!conv_out1(ha, dec6_.w, dec6_.b, pcm_dev, (int)T, dec6_.ic, dec6_.k, s, nb_)) return false;
        *n_out = T;
        return true;
    }
    ConvParams p6;
    p6.xh = ha; p6.T_in = (int)T; p6.C_in = dec6_.ic;
    p6.n_taps = dec6_.k;
    for (int j = 0; j < dec6_.k; ++j) p6.taps[j] = ConvTap{dec6_.w + (size_t)j * dec6_.oc * dec6_.ic, j - 6};
    p6.dmin = -6; p6.dmax = dec6_.k - 1 - 6;
    p6.y = pcm_dev; p6.C_out = dec6_.oc; p6.M = (int)T + 6 - (dec6_.k - 1); p6.bias = dec6_.b; p6.act = 1;
    p6.nb = nb_; p6.xbs = T; p6.ybs = p6.M;
    if (!conv(p6, s)) return false;
    *n_out = T;
    return true;
}

bool Vocoder::decode(const int32_t *codes, int F, int mode, float *pcm, int64_t *n_out, int chunk_frames) {
    *n_out = n_samples(F, mode);
    if (F <= 0) return true;
    if (mode == 0) {
        if (!ensure(F)) return false;
        Q3T_HIP(hipMemcpyAsync(codes_, codes, (size_t)F * 16 * 4, hipMemcpyHostToDevice, stream_));
        int64_t n = 0;
        if (!decode_device(codes_, F, pcm_, &n, stream_)) return false;
        Q3T_HIP(hipMemcpyAsync(pcm, pcm_, (size_t)n * 4, hipMemcpyDeviceToHost, stream_));
        Q3T_HIP(hipStreamSynchronize(stream_));
        *n_out = n;
        return true;
    }
    // CHUNK40: every chunk of the utterance in shared launches
    return decode_batch(1, &codes, &F, mode, &pcm, n_out, chunk_frames);
}

bool Vocoder::decode_batch(int n_utt, const int32_t *const *codes, const int *n_frames, int mode, float *const *pcm,
                           int64_t *n_out, int chunk_frames) {
    // a sequence = one utterance (FULL) or one chunk_frames-long chunk of one (CHUNK40, trt_vocoder.cpp:98-170:
    // independent fixed-length chunks, zero-padded codes, chunk_frames*1920 samples kept)
    struct Seq { int u, off, nf; };
    std::vector<Seq> seqs;
    if (mode != 0 && chunk_frames <= 0) { set_error("vocoder: chunk_frames must be > 0"); return false; }
    for (int u = 0; u < n_utt; ++u) {
        const int nf = std::max(n_frames[u], 0);
        n_out[u] = n_samples(nf, mode);
        if (mode == 0) {
            if (nf > 0) seqs.push_back({u, 0, nf});
        } else {
            for (int off = 0; off < nf; off += chunk_frames) seqs.push_back({u, off, std::min(chunk_frames, nf - off)});
        }
    }
    // FULL: longest first, so each batch pads its utterances to a similar length (the decoder is causal end to end:
    // frames appended after an utterance change none of its samples)
    if (mode == 0) std::stable_sort(seqs.begin(), seqs.end(), [](const Seq &a, const Seq &b) { return a.nf > b.nf; });
    std::vector<int32_t> hc;
    for (size_t i = 0; i < seqs.size();) {
        const int F = mode == 0 ? seqs[i].nf : chunk_frames;
        const int nb = (int)std::min<size_t>(seqs.size() - i, (size_t)std::max(1, batch_frames_ / F));
        if (!ensure(F, nb)) return false;
        hc.assign((size_t)nb * F * 16, 0);
        for (int j = 0; j < nb; ++j) {
            const Seq &q = seqs[i + j];
            std::memcpy(hc.data() + (size_t)j * F * 16, codes[q.u] + (size_t)q.off * 16, (size_t)q.nf * 16 * 4);
        }
        Q3T_HIP(hipMemcpyAsync(codes_, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, stream_));
        int64_t per = 0;   // samples per sequence of this batch
        if (!decode_device(codes_, F, pcm_, &per, stream_, nb)) return false;
        for (int j = 0; j < nb; ++j) {
            const Seq &q = seqs[i + j];
            const float *src = pcm_ + (size_t)j * per;
            if (mode == 0) {
                Q3T_HIP(hipMemcpyAsync(pcm[q.u], src, (size_t)n_out[q.u] * 4, hipMemcpyDeviceToHost, stream_));
            } else {
                const int64_t want = (int64_t)q.nf * 1920, have = std::min(want, per);
                Q3T_HIP(hipMemcpyAsync(pcm[q.u] + (size_t)q.off * 1920, src, (size_t)have * 4, hipMemcpyDeviceToHost, stream_));
                for (int64_t k = have; k < want; ++k) pcm[q.u][(size_t)q.off * 1920 + k] = 0.0f;
            }
        }
        Q3T_HIP(hipStreamSynchronize(stream_));
        i += nb;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ streaming decode
Vocoder::Stream *Vocoder::stream_open(int max_frames, int halo) {
    if (!loaded_) { set_error("vocoder not loaded"); return nullptr; }
    if (max_frames <= 0) { set_error("vocoder stream: max_frames must be > 0"); return nullptr; }
    if (halo < 0) {
        halo = stream_halo();
        if (const char *e = std::getenv("Q3T_VOC_STREAM_HALO")) halo = std::atoi(e);
    }
    // a push starts `lead` samples before its first frame's boundary: the window must reach at least that far back
    const int64_t rate = full_len(2) - full_len(1), lead = rate - full_len(1);
    halo = std::max<int>(halo, lead > 0 ? (int)((lead + rate - 1) / rate) : 0);
    halo = std::min(halo, max_frames);
    const size_t L = layers_.size(), LAT = latent_;
    const size_t kv = L * (size_t)max_frames * LAT * 4;
    Stream *st = new Stream();
    st->owner = this;
    st->max_frames = max_frames;
    st->halo = halo;
    auto alloc = [&](size_t bytes) -> float * {
        void *p = nullptr;
        return hipMalloc(&p, std::max<size_t>(bytes, 16)) == hipSuccess ? (float *)p : nullptr;
    };
    st->kc = alloc(kv);
    st->vc = alloc(kv);
    st->rope = alloc((size_t)max_frames * head_dim_ * 4);
    st->rvq_tail = alloc((size_t)2 * hidden_ * 4);
    st->halo_rows = alloc((size_t)halo * LAT * 4);
    if (!st->kc || !st->vc || !st->rope || !st->rvq_tail || !st->halo_rows) {
        (void)hipGetLastError();
        stream_close(st);
        set_error("vocoder stream: cannot allocate the state of " + std::to_string(max_frames) + " frames (" +
                  std::to_string((2 * kv) >> 20) + " MB of K/V cache)");
        return nullptr;
    }
    // RoPE cos/sin by absolute position, the recurrence of ensure() (ggml_rope_cache_init)
    std::vector<float> rope((size_t)max_frames * head_dim_);
    const float theta_scale = powf(10000.0f, -2.0f / (float)head_dim_);
    for (int p = 0; p < max_frames; ++p) {
        float theta = (float)p;
        for (int i0 = 0; i0 < head_dim_; i0 += 2) {
            rope[(size_t)p * head_dim_ + i0] = cosf(theta);
            rope[(size_t)p * head_dim_ + i0 + 1] = sinf(theta);
            theta *= theta_scale;
        }
    }
    if (hipMemcpy(st->rope, rope.data(), rope.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        stream_close(st);
        set_error("vocoder stream: rope upload failed");
        return nullptr;
    }
    streams_.push_back(st);
    return st;
}

void Vocoder::stream_close(Stream *st) {
    if (!st) return;
    streams_.erase(std::remove(streams_.begin(), streams_.end(), st), streams_.end());
    if (stream_) hipStreamSynchronize(stream_);   // a push in flight on the decoder's stream reads the state
    for (float *p : {st->kc, st->vc, st->rope, st->rvq_tail, st->halo_rows, st->out_hist})
        if (p) hipFree(p);
    delete st;
}

bool Vocoder::stream_reset(Stream *st) {
    if (!st || std::find(streams_.begin(), streams_.end(), st) == streams_.end()) { set_error("vocoder stream: not an open stream"); return false; }
    // pushes synchronise before they return, so nothing in flight reads the counters
    st->frames = 0;
    st->samples = 0;
    // the output stage keeps its spec and starts over: zero history, no samples, open for pushes again
    if (st->has_out) Q3T_HIP(hipMemsetAsync(st->out_hist, 0, kPcmMaxHist * sizeof(float), stream_));
    st->out_samples = 0;
    st->out_final = false;
    st->out_stale = false;
    return true;
}

bool Vocoder::stream_push(Stream *st, const int32_t *codes, int n, float *pcm, int64_t pcm_cap, int64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!st || std::find(streams_.begin(), streams_.end(), st) == streams_.end()) { set_error("vocoder stream: not an open stream"); return false; }
    if (st->has_out) { set_error("vocoder stream: the stream has an output spec (use q3t_vocoder_stream_push_out)"); return false; }
    if (n <= 0) { set_error("vocoder stream: n_frames must be > 0"); return false; }
    if (!codes || !pcm) { set_error("null argument"); return false; }
    const int P = st->frames;
    if ((int64_t)P + n > st->max_frames) {
        set_error("vocoder stream: push of " + std::to_string(n) + " frames after " + std::to_string(P) +
                  " exceeds max_frames " + std::to_string(st->max_frames));
        return false;
    }
    const int64_t total = full_len(P + n), count = std::max<int64_t>(total - st->samples, 0);
    if (pcm_cap < count) {
        set_error("vocoder stream: pcm_cap " + std::to_string(pcm_cap) + " < " + std::to_string(count) + " samples of this push");
        return false;
    }
    const int hrows = std::min(st->halo, P), W = hrows + n;   // window of the convolution stack, from frame P - hrows
    if (!ensure(std::max(W, n + 2))) return false;
    Q3T_HIP(hipMemcpyAsync(codes_, codes, (size_t)n * 16 * 4, hipMemcpyHostToDevice, stream_));
    nb_ = 1;
    int64_t nwin = 0;
    if (!frame_rows(codes_, n, stream_, st)) return false;
    // from here on the stream's state is that of P + n frames
    st->frames = P + n;
    st->samples = total;
    if (!conv_stack(W, pcm_, &nwin, stream_)) return false;
    // the window's decode is the full decode shifted by (P - hrows) * rate samples: keep what follows the samples
    // already emitted
    const int64_t rate = full_len(2) - full_len(1);
    const int64_t off = (total - count) - (int64_t)(P - hrows) * rate;
    if (off < 0 || off + count != nwin) { set_error("vocoder stream: window bookkeeping"); return false; }
    if (count) Q3T_HIP(hipMemcpyAsync(pcm, pcm_ + off, (size_t)count * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    if (n_out) *n_out = count;
    return true;
}

bool Vocoder::stream_push_batch(int S, Stream *const *sts, const int32_t *const *codes, const int32_t *n_frames,
                                float *const *pcm, const int64_t *pcm_cap, int64_t *n_out) {
    return push_batch(S, sts, codes, n_frames, pcm, pcm_cap, n_out, nullptr);
}

bool Vocoder::stream_push_batch_out(int S, Stream *const *sts, const int32_t *const *codes, const int32_t *n_frames,
                                    const int32_t *final, void *const *out, const int64_t *out_cap_bytes, int64_t *n_out) {
    const OutReq req{final, out, out_cap_bytes};
    return push_batch(S, sts, codes, n_frames, nullptr, nullptr, n_out, &req);
}

// oreq == nullptr: the plain batched push (f32 at the native rate into pcm).  oreq: the same launches with the
// convolution stack's samples kept on the device, then the output stage over all streams
bool Vocoder::push_batch(int S, Stream *const *sts, const int32_t *const *codes, const int32_t *n_frames,
                         float *const *pcm, const int64_t *pcm_cap, int64_t *n_out, const OutReq *oreq) {
    last_groups_ = 0;
    if (n_out) for (int j = 0; j < S; ++j) n_out[j] = 0;
    if (S <= 0) { set_error("vocoder stream batch: n_streams must be > 0"); return false; }
    if (!sts || !codes || !n_frames || !n_out) { set_error("null argument"); return false; }
    if (oreq ? (!oreq->final || !oreq->out || !oreq->cap) : (!pcm || !pcm_cap)) { set_error("null argument"); return false; }
    // ---- validation: nothing below this block fails on an argument
    struct Item {
        Stream *st;
        int P, n, tail, hrows;   // position, new frames, carried RVQ rows, carried output_proj rows
        int row0;                // first of its rows in the packed row-wise buffers
        size_t wa, wh;           // first row of its pre_conv window / convolution-stack window among all windows
        int64_t total, count;    // samples after the push, samples of the push
        // output stage: its tap table, outputs of the push, first byte in po_bytes_, first sample in po_stage_
        const OutTaps *ot = nullptr;
        int64_t out_n = 0;
        size_t out_off = 0, stage_off = 0;
    };
    std::vector<Item> it((size_t)S);
    {
        std::vector<const Stream *> seen;
        for (int j = 0; j < S; ++j) {
            Stream *st = sts[j];
            const std::string who = "vocoder stream batch: stream " + std::to_string(j);
            if (!st || std::find(streams_.begin(), streams_.end(), st) == streams_.end()) {
                set_error(who + " is not an open stream of this decoder");
                return false;
            }
            seen.push_back(st);
            const int n = n_frames[j], P = st->frames;
            // an output push of no frames that is final only flushes the filter's tail (an utterance's last queue
            // delivery may carry no frame): it takes no part in the vocoder's launches, only in the output stage's
            const bool flush = oreq && n == 0 && oreq->final[j] != 0;
            if (n <= 0 && !flush) { set_error(who + ": n_frames must be > 0"); return false; }
            if ((!codes[j] && !flush) || !(oreq ? oreq->out[j] != nullptr : pcm[j] != nullptr)) { set_error(who + ": null argument"); return false; }
            if (!oreq && st->has_out) { set_error(who + " has an output spec (use q3t_vocoder_stream_push_batch_out)"); return false; }
            if (oreq && !st->has_out) { set_error(who + " has no output spec (q3t_vocoder_stream_set_output)"); return false; }
            if (oreq && st->out_stale) { set_error(who + ": an earlier output push failed after its frames were taken (reset the stream first)"); return false; }
            if (oreq && st->out_final) { set_error(who + ": push after a final push (reset the stream first)"); return false; }
            if ((int64_t)P + n > st->max_frames) {
                set_error(who + ": push of " + std::to_string(n) + " frames after " + std::to_string(P) +
                          " exceeds max_frames " + std::to_string(st->max_frames));
                return false;
            }
            Item &q = it[j];
            q.st = st; q.P = P; q.n = n; q.tail = std::min(2, P); q.hrows = std::min(st->halo, P);
            q.total = full_len(P + n);
            q.count = std::max<int64_t>(q.total - st->samples, 0);
            if (oreq) {
                q.out_n = pcm_num_samples(q.total, st->out_rate, oreq->final[j] != 0) - st->out_samples;
                const int64_t bytes = q.out_n * pcm_bytes_per_sample(st->out_format);
                if (oreq->cap[j] < bytes) {
                    set_error(who + ": out_cap_bytes " + std::to_string(oreq->cap[j]) + " < " + std::to_string(bytes) +
                              " bytes of this push");
                    return false;
                }
            } else if (pcm_cap[j] < q.count) {
                set_error(who + ": pcm_cap " + std::to_string(pcm_cap[j]) + " < " + std::to_string(q.count) +
                          " samples of this push");
                return false;
            }
        }
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) {
            set_error("vocoder stream batch: a stream is given twice");
            return false;
        }
    }
    // ---- groups: streams whose pre_conv window (tail + n rows) and convolution-stack window (hrows + n rows) have the
    // same lengths share those launch sequences, one sequence per grid z.  A window is never padded on the left: the
    // biases make zero rows differ from the true left edge.  A group is split only at batch_frames() window rows.
    std::vector<int> act;   // the streams that push frames (all of them, but for flush-only output pushes)
    for (int j = 0; j < S; ++j) if (it[j].n > 0) act.push_back(j);
    const int SA = (int)act.size();
    std::vector<int> ord = act;
    auto key_less = [&](int a, int b) {
        const Item &x = it[a], &y = it[b];
        if (x.n != y.n) return x.n < y.n;
        if (x.hrows != y.hrows) return x.hrows < y.hrows;
        return x.tail < y.tail;
    };
    std::stable_sort(ord.begin(), ord.end(), key_less);
    struct Group { int first, nb; };   // ord[first .. first+nb-1]
    std::vector<Group> groups;
    for (int i = 0; i < SA;) {
        const Item &q = it[ord[i]];
        const int cap = std::max(1, batch_frames_ / (q.hrows + q.n));
        int nb = 1;
        while (i + nb < SA && nb < cap && !key_less(ord[i], ord[i + nb])) ++nb;
        groups.push_back({i, nb});
        i += nb;
    }
    size_t R = 0, WA = 0, WH = 0;   // packed rows, pre_conv window rows, convolution-stack window rows
    int max_n = 0, max_tiles = 0;
    for (int j : act) {
        it[j].row0 = (int)R;
        R += (size_t)it[j].n;
        max_n = std::max(max_n, it[j].n);
        max_tiles = std::max(max_tiles, (it[j].P + it[j].n + 31) / 32 - it[j].P / 32);
    }
    for (int i = 0; i < SA; ++i) {
        Item &q = it[ord[i]];
        q.wa = WA; q.wh = WH;
        WA += (size_t)(q.tail + q.n);
        WH += (size_t)(q.hrows + q.n);
    }
    if (R > (size_t)1 << 30) { set_error("vocoder stream batch: too many frames in one call"); return false; }
    // ---- scratch: every growth before the first launch (ensure() frees what it replaces)
    for (const Group &g : groups) {
        const Item &q = it[ord[g.first]];
        if (!ensure(std::max(q.hrows + q.n, q.n + 2), g.nb, WA)) return false;
    }
    if (oreq) {   // the stage's tables and scratch: sized from the windows, every growth before the first launch
        size_t stage = 0, bytes = 0;
        for (const Group &g : groups) {
            const Item &q0 = it[ord[g.first]];
            const size_t nwin = (size_t)full_len(q0.hrows + q0.n);
            for (int k = 0; k < g.nb; ++k) it[ord[g.first + k]].stage_off = stage + (size_t)k * nwin;
            stage += (size_t)g.nb * nwin;
        }
        for (Item &q : it) {
            if (!(q.ot = out_taps(q.st->out_rate))) return false;
            q.out_off = bytes;
            bytes += ((size_t)q.out_n * pcm_bytes_per_sample(q.st->out_format) + 15) / 16 * 16;
        }
        if (!out_scratch(stage, bytes, (size_t)S)) return false;
    }
    const int VH = hidden_, LAT = latent_;
    const size_t n_copy = 7 * (size_t)S;
    const size_t desc_bytes = (size_t)S * sizeof(VocStreamDesc) + n_copy * sizeof(VocCopyDesc);
    if (WH * LAT > sb_win_cap_) {
        if (sb_win_) hipFree(sb_win_);
        sb_win_ = nullptr; sb_win_cap_ = 0;
        void *p = nullptr;
        if (hipMalloc(&p, WH * LAT * 4) != hipSuccess) { (void)hipGetLastError(); set_error("vocoder stream batch: window alloc"); return false; }
        sb_win_ = (float *)p; sb_win_cap_ = WH * LAT;
    }
    if (desc_bytes > sb_desc_cap_) {
        if (sb_desc_) hipFree(sb_desc_);
        sb_desc_ = nullptr; sb_desc_cap_ = 0;
        if (hipMalloc(&sb_desc_, desc_bytes) != hipSuccess) { (void)hipGetLastError(); sb_desc_ = nullptr; set_error("vocoder stream batch: descriptor alloc"); return false; }
        sb_desc_cap_ = desc_bytes;
    }
    float *A = buf_[0], *B = buf_[1], *C = buf_[2], *WIN = sb_win_;
    // ---- descriptors of the whole call, one upload: the attention's per stream, then the five copy launches'
    std::vector<VocStreamDesc> sd((size_t)S);
    std::vector<VocCopyDesc> cd;
    cd.reserve(n_copy);
    struct Span { size_t first = 0; int count = 0; int64_t max_n = 0; } sp[5];
    auto add = [&](Span &spn, const float *src, float *dst, size_t nfl) {
        if (!nfl) return;
        if (!spn.count) spn.first = cd.size();
        cd.push_back(VocCopyDesc{src, dst, (int64_t)nfl});
        ++spn.count;
        spn.max_n = std::max<int64_t>(spn.max_n, (int64_t)nfl);
    };
    for (int a = 0; a < SA; ++a) {
        const Item &q = it[act[a]];
        Stream *st = q.st;
        sd[a].kc = st->kc; sd[a].vc = st->vc; sd[a].rope = st->rope;
        sd[a].layer_stride = (int64_t)st->max_frames * LAT;
        sd[a].P = q.P; sd[a].n = q.n; sd[a].row0 = q.row0;
    }
    for (int j : act) {   // 0: [tail | new RVQ rows] windows in A, from the state and the packed rows in C
        const Item &q = it[j];
        add(sp[0], q.st->rvq_tail, A + q.wa * VH, (size_t)q.tail * VH);
        add(sp[0], C + (size_t)q.row0 * VH, A + (q.wa + q.tail) * VH, (size_t)q.n * VH);
    }
    for (int j : act) {   // 1: the next push's tail, the last rows of the window
        const Item &q = it[j];
        const int keep = std::min(2, q.P + q.n);
        add(sp[1], A + (q.wa + q.tail + q.n - keep) * VH, q.st->rvq_tail, (size_t)keep * VH);
    }
    for (int j : act) {   // 2: pre_conv's rows of the new frames (windows in B), packed into C
        const Item &q = it[j];
        add(sp[2], B + (q.wa + q.tail) * LAT, C + (size_t)q.row0 * LAT, (size_t)q.n * LAT);
    }
    for (int j : act) {   // 3: [halo rows | new output_proj rows] windows, from the state and the packed rows in C
        const Item &q = it[j];
        add(sp[3], q.st->halo_rows, WIN + q.wh * LAT, (size_t)q.hrows * LAT);
        add(sp[3], C + (size_t)q.row0 * LAT, WIN + (q.wh + q.hrows) * LAT, (size_t)q.n * LAT);
    }
    for (int j : act) {   // 4: the next push's halo, the last rows of the window
        const Item &q = it[j];
        const int keep = std::min(q.st->halo, q.P + q.n);
        add(sp[4], WIN + (q.wh + q.hrows + q.n - keep) * LAT, q.st->halo_rows, (size_t)keep * LAT);
    }
    std::vector<unsigned char> hd(desc_bytes, 0);
    std::memcpy(hd.data(), sd.data(), sd.size() * sizeof(VocStreamDesc));
    std::memcpy(hd.data() + (size_t)S * sizeof(VocStreamDesc), cd.data(), cd.size() * sizeof(VocCopyDesc));
    const VocStreamDesc *dsd = static_cast<const VocStreamDesc *>(sb_desc_);
    const VocCopyDesc *dcd = reinterpret_cast<const VocCopyDesc *>(static_cast<const unsigned char *>(sb_desc_) +
                                                                   (size_t)S * sizeof(VocStreamDesc));
    const bool vec4 = VH % 4 == 0 && LAT % 4 == 0;
    hipStream_t s = stream_;
    auto copies = [&](const Span &spn) { return voc_copy_batch(dcd + spn.first, spn.count, spn.max_n, vec4, s); };
    std::vector<int32_t> hc(R * 16);
    for (int j : act) std::memcpy(hc.data() + (size_t)it[j].row0 * 16, codes[j], (size_t)it[j].n * 16 * 4);
    if (SA > 0) {
        Q3T_HIP(hipMemcpyAsync(codes_, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, s));
        Q3T_HIP(hipMemcpyAsync(sb_desc_, hd.data(), desc_bytes, hipMemcpyHostToDevice, s));
        // ---- frame-rate half: frame_rows' stages, the row-wise ones over all R rows at once
        nb_ = 1;
        if (!rvq_rows(codes_, (int)R, C, s) || !copies(sp[0]) || !copies(sp[1])) return false;
        for (const Group &g : groups) {
            const Item &q = it[ord[g.first]];
            nb_ = g.nb;
            const bool ok = run_conv(pre_conv_, A + q.wa * VH, q.tail + q.n, 2, 1, nullptr, B + q.wa * LAT, nullptr, 0, s);
            nb_ = 1;
            if (!ok) return false;
        }
        if (!copies(sp[2])) return false;
        auto attn = [&](int layer, float *qkv, uint16_t *att) {
            return voc_kv_append_batch(qkv, dsd, SA, max_n, layer, n_heads_, head_dim_, s) &&
                   voc_attn_cached_batch(qkv, att, dsd, SA, max_tiles, layer, n_heads_, head_dim_, s);
        };
        if (!layer_rows(C, (int)R, C, s, attn) || !copies(sp[3]) || !copies(sp[4])) return false;
    }
    // from here on every stream's state is that of P + n frames
    for (Item &q : it) {
        q.st->frames = q.P + q.n;
        q.st->samples = q.total;
        if (oreq) q.st->out_stale = true;   // until the stage has run: a failure below leaves the stream in need of a reset
    }
    // ---- convolution half: one launch sequence per group, its windows copied to where conv_stack reads them
    const int64_t rate = full_len(2) - full_len(1);
    for (const Group &g : groups) {
        const Item &q0 = it[ord[g.first]];
        const int W = q0.hrows + q0.n;
        Q3T_HIP(hipMemcpyAsync(B, WIN + q0.wh * LAT, (size_t)g.nb * W * LAT * 4, hipMemcpyDeviceToDevice, s));
        int64_t nwin = 0;
        nb_ = g.nb;
        // with an output stage the group's samples stay on the device, each group in its own part of po_stage_
        const bool ok = conv_stack(W, oreq ? po_stage_ + q0.stage_off : pcm_, &nwin, s);
        nb_ = 1;
        if (!ok) return false;
        ++last_groups_;
        for (int k = 0; k < g.nb; ++k) {
            const int j = ord[g.first + k];
            Item &q = it[j];
            // as in stream_push: the window's decode is the full decode shifted by (P - hrows) * rate samples
            const int64_t off = (q.total - q.count) - (int64_t)(q.P - q.hrows) * rate;
            if (off < 0 || off + q.count != nwin || (oreq && nwin != full_len(W))) { set_error("vocoder stream: window bookkeeping"); return false; }
            if (oreq) q.stage_off += (size_t)off;   // the push's first new sample
            else if (q.count)
                Q3T_HIP(hipMemcpyAsync(pcm[j], pcm_ + (size_t)k * nwin + off, (size_t)q.count * 4, hipMemcpyDeviceToHost, s));
        }
    }
    if (oreq) {
        // ---- output stage: one launch over every stream's new samples, the history update, the bytes back
        std::vector<PcmOutDesc> od((size_t)S);
        int64_t max_out = 0;
        for (int j = 0; j < S; ++j) {
            const Item &q = it[j];
            const Stream *st = q.st;
            PcmOutDesc &d = od[j];
            d.x = po_stage_ + q.stage_off; d.hist = st->out_hist; d.taps = q.ot->taps;
            d.out = po_bytes_ + q.out_off;
            d.s0 = q.total - q.count; d.n0 = st->out_samples;
            d.n_in = (int32_t)q.count; d.n_out = (int32_t)q.out_n;
            d.n_zero = oreq->final[j] ? q.ot->geo.D : 0;
            d.L = q.ot->geo.L; d.M = q.ot->geo.M; d.K = q.ot->geo.K; d.format = st->out_format;
            max_out = std::max(max_out, q.out_n);
        }
        Q3T_HIP(hipMemcpyAsync(po_desc_, od.data(), od.size() * sizeof(PcmOutDesc), hipMemcpyHostToDevice, s));
        if (!pcm_out(po_desc_, S, max_out, s) || !pcm_out_hist(po_desc_, S, s)) return false;
        for (int j = 0; j < S; ++j) {
            Item &q = it[j];
            const size_t bytes = (size_t)q.out_n * pcm_bytes_per_sample(q.st->out_format);
            if (bytes) Q3T_HIP(hipMemcpyAsync(oreq->out[j], po_bytes_ + q.out_off, bytes, hipMemcpyDeviceToHost, s));
            q.st->out_samples += q.out_n;
            q.st->out_final = oreq->final[j] != 0;
        }
    }
    Q3T_HIP(hipStreamSynchronize(s));
    if (oreq) for (Item &q : it) q.st->out_stale = false;
    for (int j = 0; j < S; ++j) n_out[j] = oreq ? it[j].out_n : it[j].count;
    return true;
}

// ---------------------------------------------------------------------------------------------------- output stage
bool Vocoder::check_spec(const OutSpec &spec) {
    PcmRate g;
    if (!pcm_rate(spec.rate, &g)) {
        set_error("output sample rate " + std::to_string(spec.rate) + " is not supported (supported: " + pcm_rates_text() + ")");
        return false;
    }
    if (!pcm_bytes_per_sample(spec.format)) {
        set_error("output format " + std::to_string(spec.format) + " is not supported (0 = f32, 1 = s16, 2 = mu-law)");
        return false;
    }
    return true;
}

// the device tap table of a rate, built once per decoder on first use
const Vocoder::OutTaps *Vocoder::out_taps(int rate) {
    for (const OutTaps &t : out_taps_) if (t.rate == rate) return &t;
    OutTaps t;
    std::vector<float> h;
    t.rate = rate;
    if (!pcm_taps(rate, &t.geo, &h)) { set_error("output sample rate " + std::to_string(rate) + " is not supported"); return nullptr; }
    if (t.geo.K - 1 > kPcmMaxHist || t.geo.M > 3 * t.geo.L) { set_error("output stage: filter geometry out of range"); return nullptr; }
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(h.size() * 4, 16)) != hipSuccess ||
        (!h.empty() && hipMemcpy(p, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipGetLastError();
        if (p) hipFree(p);
        set_error("output stage: tap table upload failed");
        return nullptr;
    }
    t.taps = (float *)p;
    out_taps_.reserve(8);   // one per supported rate: pointers handed out stay valid
    out_taps_.push_back(t);
    return &out_taps_.back();
}

bool Vocoder::out_scratch(size_t stage_floats, size_t out_bytes, size_t n_desc) {
    auto grow = [&](void **p, size_t *cap, size_t want, size_t elem) {
        if (want <= *cap && *p) return true;
        if (*p) { hipStreamSynchronize(stream_); hipFree(*p); }
        *p = nullptr; *cap = 0;
        if (hipMalloc(p, std::max<size_t>(want * elem, 16)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; set_error("output stage: scratch alloc"); return false; }
        *cap = want;
        return true;
    };
    if (!po_hist0_) {
        void *p = nullptr;
        if (hipMalloc(&p, kPcmMaxHist * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); set_error("output stage: scratch alloc"); return false; }
        po_hist0_ = (float *)p;
    }
    return grow((void **)&po_stage_, &po_stage_cap_, stage_floats, 4) && grow((void **)&po_bytes_, &po_bytes_cap_, out_bytes, 1) &&
           grow((void **)&po_desc_, &po_desc_cap_, n_desc, sizeof(PcmOutDesc));
}

bool Vocoder::stream_set_output(Stream *st, const OutSpec *spec) {
    if (!st || std::find(streams_.begin(), streams_.end(), st) == streams_.end()) { set_error("vocoder stream: not an open stream"); return false; }
    if (st->frames != 0) {
        set_error("vocoder stream: the output spec can be set only at zero frames (the stream has " + std::to_string(st->frames) + ")");
        return false;
    }
    if (!spec) {
        st->has_out = false;
        st->out_samples = 0;
        st->out_final = false;
        st->out_stale = false;
        return true;
    }
    if (!check_spec(*spec) || !out_taps(spec->rate)) return false;
    if (!st->out_hist) {
        void *p = nullptr;
        if (hipMalloc(&p, kPcmMaxHist * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); set_error("vocoder stream: output history alloc"); return false; }
        st->out_hist = (float *)p;
    }
    Q3T_HIP(hipMemsetAsync(st->out_hist, 0, kPcmMaxHist * sizeof(float), stream_));
    st->has_out = true;
    st->out_rate = spec->rate; st->out_format = spec->format;
    st->out_samples = 0;
    st->out_final = false;
    st->out_stale = false;
    return true;
}

bool Vocoder::decode_out(const int32_t *codes, int F, int mode, const OutSpec &spec, void *out, int64_t out_cap_bytes,
                         int64_t *n_out, int chunk_frames) {
    if (n_out) *n_out = 0;
    if (!check_spec(spec)) return false;
    const OutTaps *ot = out_taps(spec.rate);
    if (!ot) return false;
    const int64_t n_in = n_samples(F, mode), n = pcm_num_samples(n_in, spec.rate, true);
    const size_t bytes = (size_t)n * pcm_bytes_per_sample(spec.format);
    if (out_cap_bytes < (int64_t)bytes) {
        set_error("vocoder: out_cap_bytes " + std::to_string(out_cap_bytes) + " < " + std::to_string(bytes) + " bytes of this decode");
        return false;
    }
    if (n > 0 && !out) { set_error("null argument"); return false; }
    if (n_in >= ((int64_t)1 << 31) - 1) { set_error("vocoder: too many samples for one output-stage launch"); return false; }
    if (!out_scratch(mode == 0 ? 0 : (size_t)n_in, bytes, 1)) return false;
    const float *x = nullptr;
    if (F > 0 && mode == 0) {
        if (!ensure(F)) return false;
        Q3T_HIP(hipMemcpyAsync(codes_, codes, (size_t)F * 16 * 4, hipMemcpyHostToDevice, stream_));
        int64_t got = 0;
        if (!decode_device(codes_, F, pcm_, &got, stream_)) return false;
        if (got != n_in) { set_error("vocoder: sample count bookkeeping"); return false; }
        x = pcm_;
    } else if (F > 0) {
        // CHUNK40 assembles its chunks on the host (decode_batch); the stage then runs over the assembled signal
        std::vector<float> tmp((size_t)n_in);
        int64_t got = 0;
        if (!decode(codes, F, mode, tmp.data(), &got, chunk_frames)) return false;
        if (got != n_in) { set_error("vocoder: sample count bookkeeping"); return false; }
        Q3T_HIP(hipMemcpyAsync(po_stage_, tmp.data(), (size_t)n_in * 4, hipMemcpyHostToDevice, stream_));
        x = po_stage_;
    }
    if (n > 0) {
        Q3T_HIP(hipMemsetAsync(po_hist0_, 0, kPcmMaxHist * sizeof(float), stream_));
        PcmOutDesc d;
        d.x = x; d.hist = po_hist0_; d.taps = ot->taps; d.out = po_bytes_;
        d.n_in = (int32_t)n_in; d.n_out = (int32_t)n; d.n_zero = ot->geo.D;
        d.L = ot->geo.L; d.M = ot->geo.M; d.K = ot->geo.K; d.format = spec.format;
        Q3T_HIP(hipMemcpyAsync(po_desc_, &d, sizeof d, hipMemcpyHostToDevice, stream_));
        if (!pcm_out(po_desc_, 1, n, stream_)) return false;
        Q3T_HIP(hipMemcpyAsync(out, po_bytes_, bytes, hipMemcpyDeviceToHost, stream_));
    }
    Q3T_HIP(hipStreamSynchronize(stream_));
    if (n_out) *n_out = n;
    return true;
}

}  // namespace q3t
